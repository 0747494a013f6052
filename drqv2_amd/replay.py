"""Device-resident replay store and batch assembly.

The reference keeps episodes as numpy dicts in DataLoader workers and ships every batch host -> pinned ->
device (`replay_buffer.py:76-190`): 32.5 MB per update at batch 256, which caps training at the PCIe rate.
Here the steps live in HBM (uint8 frames: 63,504 B per step, 1 M steps = 63.5 GB of the 288 GB) and
`drq_nstep_gather` (one launch) assembles the batch in place: two frame gathers, the action rows and the
n-step reward/discount accumulation of `_sample` (`replay_buffer.py:142-160`) in the reference's float32 order.

Semantics kept from the reference: episodes are stored whole, each with its dummy first transition; eviction
drops the OLDEST whole episodes until the new one fits (`_store_episode`, :100-118); a sample picks an episode
uniformly, then `idx` uniformly in [1, len - nstep + 1] (:145-150).  Not kept: the on-disk npz files and the
worker processes (their per-worker RNG streams are not reproducible in the reference either); index draws come
from one numpy RandomState, vectorised over the batch.

Prioritized replay (new: `priority_alpha`; the reference samples uniformly).  Proportional prioritization (Schaul et
al. 2016): position i is drawn with probability p_i^alpha / sum_k p_k^alpha, stratified over the batch, and carries the
importance weight (N P(i))^-beta / max_batch.  The priorities live in a sum tree in HBM (csrc/per.hip, the layout is in
include/drqv2_hip.h); a draw is one launch (drq_per_sample) whose positions never leave the device, the new priorities
|TD error| come out of the update's own loss launch and go back into the tree with one more (drq_per_update).  The
host only counts: which slots can be drawn, how many there are, how many episodes have been placed.

Vectorised collection (new: VecDeviceReplay, csrc/vecreplay.hip).  N environments stepped in lockstep write one row per
step into a ring, straight from device tensors; episode boundaries are flags on the device, an n-step window ends at
one, and the batches are the IndexedBatch above.  The episode store and everything it does are unchanged.  With
`priority_alpha` the ring carries the same sum tree over its slots, kept and drawn from entirely on the device.

Single frames (new: VecFrameReplay, csrc/vecframes.hip).  The same ring with ONE 3 x 84 x 84 frame per slot instead of the
three-frame stack: a third of the memory and of add()'s traffic.  The stack is put together where it is read -- by the
fused aug+conv1 launch of update() (a FrameBatch carries the ring's flags), by observation() for act_batch(), by
materialize() -- following the reset rule of the reference's FrameStackWrapper (dmc.py:87-109).

Renderer images (new: VecFrameReplay.add_render, csrc/vecrender.hip).  add() for the channels-last image of S x S pixels
a GPU renderer hands out, S = 84 .. 336: one launch resizes it into the slot with an exact integer area average instead
of a chain of torch ops in front of add().

Single frames in the episode store (new: DeviceReplay(single_frames=True)).  The episode store is that ring with N = 1:
episodes are contiguous, a `first` byte marks the slot each one starts on.  add_episode() keeps the newest frame of every
step, indexed batches are FrameBatch objects, materialised ones come from one launch (drq_nstep_gather_frames).

Episode statistics (new: VecEpisodeStats, csrc/vecstats.hip).  The reference's episode_reward / episode_step book-keeping
(train.py:133,186,189) for N lockstep environments, kept on the device from the reward and first tensors add() takes: one
launch per step, a pinned host mirror that nothing waits for, and a per-environment episode limit for evaluation.

Checkpoints (new: state_dict() / load_state_dict() on VecDeviceReplay, VecFrameReplay, BatchIterator and VecEpisodeStats;
drqv2_amd/checkpoint.py puts them into one file with the agent and the generators).  A restored loop continues bit for
bit as the uninterrupted one would have.  The episode store keeps the reference's way: episodes are its unit.

Episode files for the ring (new: export_episodes() / add_episodes() on VecDeviceReplay and VecFrameReplay,
csrc/vecepisodes.hip, host planning in drqv2_amd/episodes.py).  What N environments collected leaves the ring as the
reference's `<timestamp>_<idx>_<len>.npz` files, which make_replay_loader() and the reference's own tooling read; and a
ring of any shape starts from such files or from episode dicts, laid out as lockstep rows and written with one launch per
staging chunk instead of one add() per row.

Demonstrations (new: VecDeviceReplay(demo_rows=D), add_demonstrations(), demo_fraction; drq_vec_sample_mixed in
csrc/vecreplay.hip).  D rows behind the ring's last row, in the same allocation, hold demonstration episodes for the whole
run: never evicted, filled by drq_vec_fill, and drawn from for a fixed share of every batch by one launch that writes slot
indices into the whole allocation -- so update() and its kernels see an IndexedBatch like any other.
"""
import collections
import datetime
import pathlib

import numpy as np
import torch

from . import _lib
from . import episodes as _episodes
from ._lib import launch, ptr
from .checkpoint import check_state, host

ExportReport = collections.namedtuple("ExportReport", "files episodes transitions next_row zero_length headless open short")
ExportReport.__doc__ = """What export_episodes() did: files (the paths written, in order), episodes and transitions (how many
of each they hold), next_row (pass it as start_row next time), and how many runs were left out as zero_length, headless,
open and short (drqv2_amd.episodes.plan_export says what each means)."""
FillReport = collections.namedtuple("FillReport", "episodes transitions rows pad_rows")
FillReport.__doc__ = """What add_episodes() did: episodes and transitions placed, rows added to the ring (T grew by that), and
pad_rows, the reset rows that fill the shorter lanes (counted over all environments)."""


class IndexedBatch(tuple):
    """A replay batch whose frames stay in the store: the 5-tuple (obs, action, reward, discount, next_obs) of the
    reference's loader with obs / next_obs replaced by int64 index tensors [B] into `frames` (the store, [slots, frame
    bytes] uint8).  DrQV2Agent.update() hands store + indices to the fused aug+conv1 launch, which gathers its source
    rows itself: the 32.5 MB batch copy (and its re-read) of the materialised form never happens."""

    def __new__(cls, frames, obs_idx, action, reward, discount, next_idx):
        self = super().__new__(cls, (obs_idx, action, reward, discount, next_idx))
        self.frames = frames
        return self

    def materialize(self, obs_shape):
        """The batch as the reference's loader would hand it over: (obs, action, reward, discount, next_obs) tensors."""
        obs_idx, action, reward, discount, next_idx = self
        shp = (obs_idx.numel(),) + tuple(obs_shape)
        return (self.frames[obs_idx].view(shp), action, reward, discount, self.frames[next_idx].view(shp))


class FrameBatch(IndexedBatch):
    """An IndexedBatch drawn from a ring of SINGLE frames (VecFrameReplay, or DeviceReplay(single_frames=True): R = its
    capacity, N = 1): obs / next_obs are the slots of the newest frame of each stack, and the batch also carries the
    ring -- `ring` = (first, R, N): the reset flags uint8 [R N] on the device and the ring's shape.  DrQV2Agent.update()
    hands all of it to the fused aug+conv1 launch, which gathers every 9-channel stack from three slots
    (drq_update_phase_frames); the stacks are never materialised."""

    def __new__(cls, frames, obs_idx, action, reward, discount, next_idx, first, R, N):
        self = super().__new__(cls, frames, obs_idx, action, reward, discount, next_idx)
        self.ring = (first, int(R), int(N))
        return self

    def stacks(self, slots, out=None):
        """uint8 [n, 3 * frame bytes]: the stacks whose newest frames are `slots` (int64 [n] on the device), one launch
        (drq_vec_stack_gather) on the current stream; out: a buffer to write into"""
        first, R, N = self.ring
        n, fb = slots.numel(), self.frames.shape[1]
        if out is None:
            out = torch.empty((n, 3 * fb), dtype=torch.uint8, device=self.frames.device)
        launch("drq_vec_stack_gather", ptr(self.frames), ptr(first), R, N, fb, ptr(slots.contiguous()), 0, n, ptr(out),
               device=self.frames.device)
        return out

    def materialize(self, obs_shape=(9, 84, 84), out=(None, None)):
        """The batch as the reference's loader would hand it over, the stacks gathered from the ring."""
        obs_idx, action, reward, discount, next_idx = self
        shp = (obs_idx.numel(),) + tuple(obs_shape)
        return (self.stacks(obs_idx, out[0]).view(shp), action, reward, discount, self.stacks(next_idx, out[1]).view(shp))


class PrioritizedBatch:
    """What a prioritized DeviceReplay yields: the batch of the store's form -- an IndexedBatch (indexed=True) or the
    materialised 5-tuple -- that also carries `weights` (float32 [B] on the device: the importance weights, largest 1)
    and `update_priorities(td_abs)`.  DrQV2Agent.update() reads both: the weights go into the critic loss, the
    per-sample TD errors the loss launch leaves come back through update_priorities, all in stream order."""

    def _per(self, store, pos, weights):
        self.weights, self._store, self._pos, self._stamp = weights, store, pos, store._stamp_now()
        return self

    def update_priorities(self, td_abs):
        """td_abs: float32 [B] on the device, the |TD error| of every row -> leaf = (td_abs + eps)^alpha.
        DeviceReplay: nothing is written if the store has placed an episode since this batch was drawn: a position of
        this batch may then lie in a newer episode, whose fresh priority must not be overwritten with an error of the
        evicted one.  VecDeviceReplay: only rows whose position is still drawable are written (one launch checks that on
        the device), and nothing if `guard_rows` or more rows were added since the draw: the batch's slots may then hold
        other transitions."""
        self._store._update_priorities(self, td_abs)


class _PrioritizedTuple(PrioritizedBatch, tuple):
    pass


class _PrioritizedIndexed(PrioritizedBatch, IndexedBatch):
    pass


class _PrioritizedFrames(PrioritizedBatch, FrameBatch):
    pass


def _rotating(cache, B, make):
    """The next of the four buffer sets a store keeps for batches of B rows in `cache` (a dict: one batch size at a
    time); make() builds one set.  Four sets, used in turn: the device tensors are written in stream order (no hazard),
    but the pinned host staging of a set is overwritten by the HOST when batch k+4 is drawn, and its upload must have run
    by then: StepEngine.update keeps at most two updates queued behind the running one (_throttle), so three batches
    can be pending at most.  A consumer of its own must bound its run-ahead likewise (or use DeviceReplay.gather())."""
    bufs = cache.get(B)
    if bufs is None:
        bufs = [make(), make(), make(), make(), 0]
        cache.clear()
        cache[B] = bufs
    cur = bufs[bufs[4]]
    bufs[4] = (bufs[4] + 1) & 3
    return cur


def _td_rows(pos, td_abs):
    """B, with td_abs checked to be the |TD error| rows of the batch drawn at the device positions pos [B]"""
    B = pos.numel()
    if (not torch.is_tensor(td_abs) or td_abs.dtype != torch.float32 or td_abs.device != pos.device
            or td_abs.numel() != B or not td_abs.is_contiguous()):
        raise _lib.DrqError(f"update_priorities(): contiguous float32 [{B}] on {pos.device} required")
    return B


def newest_frames(obs, check=True):
    """The single frames of an episode's `observation`, uint8 [T+1, 3, 84, 84] contiguous: a [T+1, 3, 84, 84] array as it
    is, of a [T+1, 9, 84, 84] array of frame stacks channels 6:9 of every step.  check: a stacked episode must be what
    the reference's FrameStackWrapper (dmc.py:87-109) builds -- the three frames of obs[0] equal, and
    obs[t][0:6] == obs[t-1][3:9] for t >= 1 -- or the frames dropped here could not be put together again: ValueError."""
    obs = np.asarray(obs)
    if obs.dtype != np.uint8 or obs.ndim != 4 or obs.shape[0] < 1 or obs.shape[1:] not in ((3, 84, 84), (9, 84, 84)):
        raise ValueError("observation must be uint8 [T+1, 9, 84, 84] frame stacks or [T+1, 3, 84, 84] single frames")
    if obs.shape[1] == 9 and check:
        if not (np.array_equal(obs[0, 0:3], obs[0, 3:6]) and np.array_equal(obs[0, 3:6], obs[0, 6:9])):
            raise ValueError("observation[0] is no reset stack: its three frames differ (dmc.py:98-103)")
        if not np.array_equal(obs[1:, 0:6], obs[:-1, 3:9]):
            t = 1 + int(np.argmax((obs[1:, 0:6] != obs[:-1, 3:9]).reshape(obs.shape[0] - 1, -1).any(axis=1)))
            raise ValueError(f"observation[{t}] is no frame stack: its two older frames are not the two newer ones of "
                             f"observation[{t - 1}] (dmc.py:105-109); check_stacks=False stores it all the same")
    return np.ascontiguousarray(obs[:, -3:])


def _on_gpu(store, what):
    if store.device.type != "cuda":
        raise _lib.DrqError(f"{what} on the GPU: the HIP path has no CPU fallback")


def _priority_args(store, priority_alpha, priority_beta, priority_eps):
    """The priority arguments of a store's constructor, checked: sets the attributes of a uniform store (no tree) and
    returns alpha as a float, or None for uniform sampling."""
    store.priority_alpha = None
    store.priority_beta, store.priority_eps = float(priority_beta), float(priority_eps)
    store.tree = None
    if priority_alpha is None:
        return None
    a = float(priority_alpha)
    if isinstance(priority_alpha, bool) or not (0.0 < a <= 1.0):
        raise ValueError(f"priority_alpha {priority_alpha!r}: None or a float in (0, 1]")
    if not (store.priority_beta >= 0.0) or not (0.0 < store.priority_eps < float("inf")):
        raise ValueError("priority_beta must be >= 0 and priority_eps > 0")
    return a


def _priority_tree(store, slots, alpha):
    """makes `store` a prioritized one: the sum tree over `slots` slots, tree[0] (the running maximum leaf: what a
    position that becomes drawable starts at) = 1"""
    _on_gpu(store, "prioritized replay keeps its sum tree")
    store.priority_alpha = alpha
    store.tree_leaves = 1 << max(0, slots - 1).bit_length()        # smallest power of two >= slots
    store.tree = torch.zeros(2 * store.tree_leaves, dtype=torch.float64, device=store.device)
    store.tree[0] = 1.0
    store._pbufs = {}


class BatchIterator:
    """Endless iterator over device batches with one batch of look-ahead: DrQV2Agent.update() calls prefetch() right
    after it has queued its kernels, so the next batch's host work (index draw, upload, gather launch) happens while the
    GPU is busy instead of in front of the next update's first launch (the reference's DataLoader workers run further
    ahead still, replay_buffer.py:173-190).  The draws and their order are those of plain next() calls."""

    def __init__(self, draw, store=None):
        """draw: the function that draws one batch.  store: the VecDeviceReplay / VecFrameReplay it draws from, which
        makes the iterator saveable (state_dict); None for any other source."""
        self._draw = draw
        self._store = store
        self._ahead = None
        self._drawn = None          # (index [3][B], steps [B]) of the look-ahead batch: the store's last_index / last_steps

    def __iter__(self):
        return self

    def __next__(self):
        b, self._ahead = self._ahead, None
        return b if b is not None else self._draw()

    def prefetch(self):
        if self._ahead is None:
            self._ahead = self._draw()
            if self._store is not None:
                self._drawn = (self._store.last_index, self._store.last_steps)

    def peek(self):
        """The look-ahead batch without consuming it (drawn now if there is none): the batch the next update() trains on,
        e.g. for DrQV2Agent.dormant_ratio()."""
        self.prefetch()
        return self._ahead

    def state_dict(self):
        """The look-ahead as a plain dict of CPU tensors and Python scalars: "format": 1, "kind", "pending", and for a
        pending batch its index tensor [3, B] (obs, next_obs and transition slots), action, reward, discount and steps,
        for a prioritized one also the weights and the stamp (the store's T at the draw).  The batch was drawn right after
        the last update() and has consumed its random numbers: drawing it again after a restore would give another, so
        it is state.  SYNCHRONISES the store's device.  DrqError: an iterator built without a store (DeviceReplay's), a
        pending batch of a store with indexed=False."""
        store = self._store
        if store is None:
            raise _lib.DrqError("BatchIterator.state_dict(): this iterator was built without a store: only the iterators "
                                "of VecDeviceReplay / VecFrameReplay can be saved")
        sd = {"format": 1, "kind": "BatchIterator", "pending": self._ahead is not None}
        if self._ahead is None:
            return sd
        if not store.indexed:
            raise _lib.DrqError("BatchIterator.state_dict(): a pending materialised batch (indexed=False) cannot be saved")
        if store.device.type == "cuda":
            torch.cuda.synchronize(store.device)
        b = self._ahead
        sd.update(index=host(self._drawn[0]), steps=host(self._drawn[1]), action=host(b[1]), reward=host(b[2]),
                  discount=host(b[3]), prioritized=isinstance(b, PrioritizedBatch))
        if sd["prioritized"]:
            sd.update(weights=host(b.weights), stamp=int(b._stamp))
        return sd

    def load_state_dict(self, sd):
        """Restores what state_dict() saved, after the store has been restored: a pending batch is rebuilt through the
        store's own batch types over the RESTORED ring -- an IndexedBatch, FrameBatch or PrioritizedBatch on the store's
        device, whose update_priorities() obeys the guard_rows rule with the saved stamp -- and becomes the store's
        last_index / last_steps, as it was when it was saved.  ValueError, with nothing changed: a wrong "format" /
        "kind", a batch that does not fit the store (its action width, its slots, uniform against prioritized)."""
        store = self._store
        if store is None:
            raise _lib.DrqError("BatchIterator.load_state_dict(): this iterator was built without a store")
        check_state(self, sd, kind="BatchIterator")
        if not sd.get("pending"):
            self._ahead = self._drawn = None
            return
        index = sd.get("index")
        if not torch.is_tensor(index) or index.dim() != 2 or index.shape[0] != 3:
            raise ValueError("BatchIterator.load_state_dict(): a pending batch needs its index tensor [3, B]")
        B, per = int(index.shape[1]), bool(sd.get("prioritized"))
        want = {"index": ((3, B), torch.int64), "steps": ((B,), torch.int32), "action": ((B, store.A), torch.float32),
                "reward": ((B, 1), torch.float32), "discount": ((B, 1), torch.float32)}
        if per:
            want["weights"] = ((B,), torch.float32)
        check_state(self, sd, tensors=want, kind="BatchIterator")
        if per != (store.tree is not None) or not store.indexed:
            raise ValueError("BatchIterator.load_state_dict(): the saved batch is "
                             f"{'prioritized' if per else 'uniform'} and indexed, the store is not")
        slots = (store.R + store.D) * store.N       # a mixed batch names slots of the demonstration partition too
        if B and not (0 <= int(index.min()) and int(index.max()) < slots):
            raise ValueError(f"BatchIterator.load_state_dict(): slots outside the ring of {slots}")
        dev = store.device
        idx, steps, act, rew, disc = (sd[k].to(dev) for k in ("index", "steps", "action", "reward", "discount"))
        batch = store._batch(per, idx, act, rew, disc)
        if per:
            batch._per(store, idx[2], sd["weights"].to(dev))
            batch._stamp = int(sd["stamp"])
        self._ahead, self._drawn = batch, (idx, steps)
        store.last_index, store.last_steps = idx, steps


class DeviceReplay:
    def __init__(self, capacity_steps, obs_shape, action_dim, nstep, discount, device, seed=None, indexed=False,
                 priority_alpha=None, priority_beta=0.4, priority_eps=1e-6, single_frames=False, check_stacks=True):
        """single_frames: False = every slot holds the whole observation, as the reference stores it.  True = a slot holds
        the ONE new 3 x 84 x 84 frame of its step (21,168 bytes instead of 63,504) and `first` (uint8 [capacity] on the
        device) marks the slot every episode starts on; obs_shape must be (9, 84, 84).  The store is then the single-frame
        ring of include/drqv2_hip.h with N = 1 and R = capacity, and whoever reads puts the stacks together: update()'s
        fused aug+conv1 launch (indexed=True yields FrameBatch objects), drq_nstep_gather_frames for the materialised
        5-tuple (indexed=False, one launch), FrameBatch.materialize().  Slots, eviction, draws and the priority tree are
        the stacked store's: same seed, same episodes, same positions.  Stale flags are harmless: those of evicted
        episodes stay where they are, but a flag is only read for slots of a live episode, at or before the slot drawn
        (positions start at the episode's slot 1); the frame two slots back is read only where the flags of the slot and
        of the one before it are both 0, two slots or more past the episode's start; an episode at slot 0 has
        first[0] = 1.  So no read leaves the episode and the ring's modulo wrap is never taken.  update() on a FrameBatch:
        single GPU, no behaviour cloning, prioritized batches in fp32 only.
        check_stacks: add_episode() verifies a stacked episode (newest_frames); False for a caller who knows the source.
        priority_alpha: None = uniform sampling (no tree is allocated, the draws from the RandomState are what they
        were); a float in (0, 1] = proportional prioritized replay, sample() yields PrioritizedBatch objects.
        priority_beta is a plain attribute, read at every draw: the training loop may anneal it towards 1.
        priority_eps (> 0) keeps a transition with zero error drawable.  The order that keeps every priority update
        valid is the one DrQV2Agent.update() and the loader's iterator follow: update, then update_priorities, then
        add_episode, then the next draw; a batch that is overtaken by an add writes no priorities (PrioritizedBatch).
        replay_buffer.make_replay_loader keeps that order by handing a prioritized store its finished episodes when the
        loader's iterator draws next, not when they finish: sample() called on the store directly does not see an
        episode the iterator has not taken over yet."""
        self.device = torch.device(device)
        self.obs_shape = tuple(int(s) for s in obs_shape)
        self.single_frames, self.check_stacks = bool(single_frames), bool(check_stacks)
        if self.single_frames and self.obs_shape != (9, 84, 84):
            raise ValueError(f"obs_shape {self.obs_shape}: a single-frame store stacks three (3, 84, 84) frames")
        self.stack_bytes = int(np.prod(self.obs_shape))            # bytes per observation
        self.frame_bytes = self.stack_bytes // 3 if self.single_frames else self.stack_bytes      # bytes per slot
        if self.frame_bytes % 16:
            raise ValueError("frame size must be a multiple of 16 bytes")
        self.A = int(action_dim)
        self.nstep = int(nstep)
        self.gamma = float(discount)
        self.capacity = int(capacity_steps)
        dev = self.device
        self.frames = torch.empty((self.capacity, self.frame_bytes), dtype=torch.uint8, device=dev)
        self.action = torch.zeros((self.capacity, self.A), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((self.capacity,), dtype=torch.float32, device=dev)
        self.discount = torch.ones((self.capacity,), dtype=torch.float32, device=dev)
        # single frames: 1 on the slot an episode starts on (the flags of the ring, include/drqv2_hip.h)
        self.first = torch.zeros((self.capacity,), dtype=torch.uint8, device=dev) if self.single_frames else None
        self.episodes = []          # [start_slot, steps (= T+1)], oldest first; each contiguous in the store
        self._head = 0              # next free slot
        self.rng = np.random.RandomState(seed)
        self._out = {}
        # True: batches are IndexedBatch objects (frames stay in the store); False: materialised tensors like the
        # reference's loader yields
        self.indexed = bool(indexed)
        self._ibufs = {}
        self._placements = 0        # episodes placed so far: what a PrioritizedBatch compares before it writes priorities
        self.n_valid = 0            # drawable positions (prioritized store)
        alpha = _priority_args(self, priority_alpha, priority_beta, priority_eps)
        if alpha is not None:
            _priority_tree(self, self.capacity, alpha)

    # ---- storage -------------------------------------------------------------------------
    def __len__(self):
        """transitions stored, as the reference counts them (episode_len = steps - 1)"""
        return sum(n - 1 for _, n in self.episodes)

    def _place(self, n):
        """slot range for an episode of n steps: contiguous, wrapping to slot 0 when the tail is too short;
        evicts every stored episode the range overlaps (they are the oldest ones).  Returns (start, the evicted
        episodes as [start, steps])."""
        if n > self.capacity:
            raise ValueError(f"episode of {n} steps exceeds the store ({self.capacity})")
        start = self._head if self._head + n <= self.capacity else 0
        end = start + n
        clear = lambda e: e[0] + e[1] <= start or e[0] >= end
        evicted = [e for e in self.episodes if not clear(e)]
        self.episodes = [e for e in self.episodes if clear(e)]
        self._head = end
        return start, evicted

    def _fill(self, lo, hi, mode):
        launch("drq_per_fill", ptr(self.tree), self.tree_leaves, lo, hi, mode, device=self.device)

    def _place_priorities(self, start, n, evicted):
        """the tree after an episode of n steps went to `start`: every slot of the evicted episodes (also the part the
        new one does not cover) and of the new one's range is 0, then the drawable positions start+1 .. start+n-nstep
        (draw_positions' range) get the running maximum"""
        for s, m in evicted:
            self._fill(s, s + m, 0)
        self._fill(start, start + n, 0)
        if n - 1 >= self.nstep:
            self._fill(start + 1, start + n - self.nstep + 1, 1)
        self.n_valid = sum(m - self.nstep for _, m in self.episodes if m - 1 >= self.nstep)

    def add_episode(self, episode):
        """episode: dict of numpy arrays like the reference's npz (observation [T+1,...] uint8, action [T+1,A],
        reward [T+1,1] or [T+1], discount likewise); index 0 is the dummy reset transition.
        A single-frame store takes observation [T+1, 9, 84, 84] (it keeps and uploads channels 6:9, after checking that
        the episode is a frame stack: a ValueError leaves the store as it was) or [T+1, 3, 84, 84] (stored as they are)."""
        if self.single_frames:
            obs = newest_frames(episode["observation"], self.check_stacks)
        else:
            obs = np.ascontiguousarray(episode["observation"])
            if obs.dtype != np.uint8 or int(np.prod(obs.shape[1:])) != self.frame_bytes:
                raise ValueError("observation must be uint8 frames of the configured shape")
        n = obs.shape[0]
        start, evicted = self._place(n)
        sl = slice(start, start + n)
        dev = self.device
        self.frames[sl].copy_(torch.from_numpy(obs.reshape(n, self.frame_bytes)), non_blocking=False)
        if self.single_frames:
            flags = np.zeros(n, np.uint8)
            flags[0] = 1
            self.first[sl].copy_(torch.from_numpy(flags))
        self.action[sl].copy_(torch.from_numpy(np.asarray(episode["action"], np.float32).reshape(n, self.A)))
        self.reward[sl].copy_(torch.from_numpy(np.asarray(episode["reward"], np.float32).reshape(n)))
        self.discount[sl].copy_(torch.from_numpy(np.asarray(episode["discount"], np.float32).reshape(n)))
        self.episodes.append([start, n])
        self._placements += 1
        if self.tree is not None:
            self._place_priorities(start, n, evicted)
        return start

    # ---- sampling ------------------------------------------------------------------------
    def draw_positions(self, batch_size):
        """store indices of `idx` for a batch: episode uniform, idx uniform in [1, len - nstep + 1]
        (replay_buffer.py:147-148).  Episodes shorter than nstep cannot be sampled (the reference would raise)."""
        ok = [(s, n) for s, n in self.episodes if n - 1 >= self.nstep]
        if not ok:
            raise _lib.DrqError("replay: no stored episode is at least nstep long")
        starts = np.array([s for s, _ in ok], np.int64)
        lens = np.array([n - 1 for _, n in ok], np.int64)
        e = self.rng.randint(0, len(ok), size=batch_size)
        idx = (self.rng.random_sample(batch_size) * (lens[e] - self.nstep + 1)).astype(np.int64) + 1
        return starts[e] + idx

    def gather(self, pos):
        """pos: int64 store indices [B] (host array or device tensor) -> (obs, action, reward, discount, next_obs) on
        the device, shaped like the reference's batch ([B,*obs], [B,A], [B,1], [B,1], [B,*obs])."""
        _on_gpu(self, "replay batch assembly runs")
        if not torch.is_tensor(pos):
            pos = torch.from_numpy(np.ascontiguousarray(pos, np.int64))
        pos = pos.to(self.device, non_blocking=True)
        B = pos.numel()
        out = self._out.get(B)
        if out is None:
            dev = self.device
            out = (torch.empty((B, self.stack_bytes), dtype=torch.uint8, device=dev),
                   torch.empty((B, self.A), dtype=torch.float32, device=dev),
                   torch.empty((B, 1), dtype=torch.float32, device=dev),
                   torch.empty((B, 1), dtype=torch.float32, device=dev),
                   torch.empty((B, self.stack_bytes), dtype=torch.uint8, device=dev))
            self._out = {B: out}            # one batch size at a time; the buffers are reused every call
        obs, act, rew, disc, nxt = out
        shp = (B,) + self.obs_shape
        if self.single_frames:              # the same batch, the stacks put together from three slots each
            launch("drq_nstep_gather_frames", ptr(self.frames), ptr(self.first), self.capacity, ptr(self.action),
                   ptr(self.reward), ptr(self.discount), ptr(pos), B, self.A, self.frame_bytes, self.nstep, self.gamma,
                   ptr(obs), ptr(act), ptr(rew), ptr(disc), ptr(nxt), device=self.device)
            return obs.view(shp), act, rew, disc, nxt.view(shp)
        launch("drq_nstep_gather", ptr(self.frames), ptr(self.action), ptr(self.reward), ptr(self.discount), ptr(pos),
               B, self.A, self.frame_bytes, self.nstep, self.gamma, ptr(obs), ptr(act), ptr(rew), ptr(disc), ptr(nxt),
               device=self.device)
        return obs.view(shp), act, rew, disc, nxt.view(shp)

    def gather_indexed(self, pos):
        """pos: host int64 store indices [B] -> IndexedBatch: action rows and n-step reward / discount assembled by the
        same kernel (its frame copies skipped), obs = frame pos-1, next_obs = frame pos+nstep-1 as indices.  A
        single-frame store yields a FrameBatch: the indices name the newest frame of each stack."""
        _on_gpu(self, "replay batch assembly runs")
        pos = np.ascontiguousarray(pos, np.int64)
        B = pos.size
        dev = self.device
        f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        idx, act, rew, disc, host = _rotating(self._ibufs, B, lambda: (
            torch.empty((3, B), dtype=torch.int64, device=dev), f(B, self.A), f(B, 1), f(B, 1),
            torch.empty((3, B), dtype=torch.int64).pin_memory()))
        h = host.numpy()
        h[0], h[1], h[2] = pos - 1, pos + self.nstep - 1, pos
        idx.copy_(host, non_blocking=True)
        launch("drq_nstep_gather", ptr(self.frames), ptr(self.action), ptr(self.reward), ptr(self.discount),
               ptr(idx[2]), B, self.A, self.frame_bytes, self.nstep, self.gamma, None, ptr(act), ptr(rew), ptr(disc),
               None, device=self.device)
        return self._batch(False, idx, act, rew, disc)

    def _batch(self, prioritized, idx, act, rew, disc):
        """the indexed batch whose slots are idx [3][B]"""
        if self.single_frames:
            return (_PrioritizedFrames if prioritized else FrameBatch)(self.frames, idx[0], act, rew, disc, idx[1],
                                                                       self.first, self.capacity, 1)
        return (_PrioritizedIndexed if prioritized else IndexedBatch)(self.frames, idx[0], act, rew, disc, idx[1])

    def sample_prioritized(self, batch_size):
        """One stratified draw on the device: u ~ U[0,1)^B from the store's RandomState (one random_sample call per
        batch) -> drq_per_sample -> drq_nstep_gather on the device positions.  Returns a PrioritizedBatch."""
        if self.n_valid <= 0:
            raise _lib.DrqError("replay: no stored episode is at least nstep long")
        B = int(batch_size)
        dev = self.device
        f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        # a set also holds the weights of its batch and, for indexed batches, their action / reward / discount rows
        # (materialised ones use gather()'s buffers)
        idx, u, w, host, rows = _rotating(self._pbufs, B, lambda: (
            torch.empty((3, B), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.float64, device=dev),
            f(B), torch.empty((B,), dtype=torch.float64).pin_memory(),
            (f(B, self.A), f(B, 1), f(B, 1)) if self.indexed else None))
        host.numpy()[:] = self.rng.random_sample(B)
        u.copy_(host, non_blocking=True)
        launch("drq_per_sample", ptr(self.tree), self.tree_leaves, ptr(u), B, self.nstep, self.n_valid,
               float(self.priority_beta), ptr(idx), ptr(w), device=self.device)
        if self.indexed:
            act, rew, disc = rows
            launch("drq_nstep_gather", ptr(self.frames), ptr(self.action), ptr(self.reward), ptr(self.discount),
                   ptr(idx[2]), B, self.A, self.frame_bytes, self.nstep, self.gamma, None, ptr(act), ptr(rew), ptr(disc),
                   None, device=self.device)
            batch = self._batch(True, idx, act, rew, disc)
        else:
            batch = _PrioritizedTuple(self.gather(idx[2]))
        return batch._per(self, idx[2], w)

    def _stamp_now(self):
        return self._placements

    def _update_priorities(self, batch, td_abs):
        if batch._stamp != self._placements:
            return                      # an episode was placed since the draw: see PrioritizedBatch.update_priorities
        pos = batch._pos
        B = _td_rows(pos, td_abs)
        launch("drq_per_update", ptr(self.tree), self.tree_leaves, ptr(pos), ptr(td_abs), B, self.priority_alpha,
               self.priority_eps, device=self.device)

    def sample(self, batch_size):
        if self.tree is not None:
            return self.sample_prioritized(batch_size)
        pos = self.draw_positions(batch_size)
        return self.gather_indexed(pos) if self.indexed else self.gather(pos)

    def __iter__(self):
        return BatchIterator(lambda: self.sample(self.batch_size))

    batch_size = 256


class VecDeviceReplay:
    """Step-major device store for N environments stepped in lockstep (new; the contract is in include/drqv2_hip.h,
    "step-major replay"): add() writes one row -- the observation after the step and the action, reward and discount that
    led to it, for all N environments -- with one launch (drq_vec_add), sample() draws, windows and indexes a batch with
    one more (drq_vec_sample).  Device tensors go in and come out; nothing here waits for the GPU or reads a flag back:
    episode boundaries are the `first` flags of the rows (1 = the dummy reset transition of a new episode, like index 0 of
    an episode file), an n-step window that meets one simply ends there (`last_steps` tells how long each window was).

    A ring of `rows` rows.  With T rows added the drawable ones are lo .. hi, hi = T - nstep and
    lo = max(1, T - rows + 1 + guard_rows): an IndexedBatch stays valid while fewer than `guard_rows` rows are added
    between its draw and the update that consumes it (the iterator's one batch of look-ahead needs 1).
    Every environment must hold a non-reset row among the drawable ones; a batch row drawn from one that does not comes
    out with steps 0, reward 0 and discount 0.  Not here: rows for a subset of the environments.

    Episode files: export_episodes() writes the episodes the ring holds whole as the reference's npz files, and
    add_episodes() fills the ring from such files or from episode dicts, one launch per staging chunk either way.

    Checkpoints: state_dict() / load_state_dict() save and restore T, the live slots of the ring, the RandomState,
    priority_beta and the whole priority tree; iter(store) is a BatchIterator that knows its store and saves its
    look-ahead batch.  A restored store draws, windows and weights exactly as the saved one would have gone on to.

    Prioritized sampling (`priority_alpha`, indexed batches only): a sum tree over the ring's slots in HBM, laid out and
    drawn from like DeviceReplay's (csrc/per.hip), maintained without the host ever reading a flag.  A leaf is positive
    exactly for the drawable, non-reset transitions.  add() makes a second launch (drq_vec_per_advance): the row that
    became drawable starts at the largest priority ever written (1 before any update), its reset rows and the row
    that stopped being drawable at 0.  sample() is one launch (drq_vec_per_sample) instead of drq_vec_sample: B
    stratified draws from one random_sample(B) call, the windows and n-step sums of the uniform draw, and the weights
    (n P(i))^-beta / max_batch with the nominal n = len(self) -- it cancels against the maximum.  The batch is a
    PrioritizedBatch; its update_priorities(td_abs) is one launch (drq_vec_per_update) that writes only positions that
    are still drawable, and nothing at all once `guard_rows` rows were added since the draw (so guard_rows >= 1 is
    needed for priorities to be renewed at all).  If every drawable row is a reset row the tree is empty, which the host
    cannot know: the batch then consists of steps-0 rows on slot(lo, 0) with weight 1.

    Demonstrations (`demo_rows=D`, uniform stores only; the contract is in include/drqv2_hip.h, "demonstrations in the
    step-major replay"): the five arrays hold (rows + D) N slots, the ring in the first rows N -- `frames`, `action`,
    `reward`, `discount` and `first` stay those views -- and behind it a partition of D rows that is linear and never
    evicted: demonstration row d of lane e in slot (rows + d) N + e.  add_demonstrations() appends episodes to it,
    `demo_rows_filled` is Td, demo_bounds() its drawable rows (1, Td - nstep).  `demo_fraction` (a plain attribute in
    [0, 1], read at every draw) makes the first Bd = int(B * demo_fraction + 0.5) rows of every batch demonstrations:
    Bd = 0 is drq_vec_sample as ever, otherwise one launch of drq_vec_sample_mixed from the same u table; `last_demo_count`
    is Bd.  A batch's `frames` is the whole allocation.  state_dict() saves Td, the fraction and the filled slots."""

    K = 4      # candidates per batch row (the columns of the u table)
    _draw_copies = True     # a materialised batch's frames are copied by the draw itself (drq_vec_sample)

    def __init__(self, rows, num_envs, obs_shape, action_dim, nstep, discount, device, seed=None, indexed=True,
                 guard_rows=8, priority_alpha=None, priority_beta=0.4, priority_eps=1e-6, demo_rows=0):
        """priority_alpha, priority_beta, priority_eps: as DeviceReplay's.  None = uniform sampling: no tree is
        allocated and every draw and launch is what it was.  priority_beta is a plain attribute, read at every draw.
        demo_rows: D rows behind the ring that hold demonstrations for the whole run (class docstring); 0 = none, and
        every allocation, launch, draw and saved state is what it was."""
        self.device = torch.device(device)
        self.obs_shape = tuple(int(s) for s in obs_shape)
        self.slot_shape = self.obs_shape           # what add() stores per environment; here the whole observation
        self.frame_bytes = self.stack_bytes = int(np.prod(self.obs_shape))     # bytes per slot, per observation
        self.R, self.N, self.A = int(rows), int(num_envs), int(action_dim)
        self.nstep, self.gamma, self.guard_rows = int(nstep), float(discount), int(guard_rows)
        self.D = int(demo_rows)
        if self.frame_bytes <= 0 or self.frame_bytes % 16:
            raise ValueError("frame size must be a multiple of 16 bytes")
        if self.N < 1 or self.A < 1 or self.nstep < 1 or self.guard_rows < 0:
            raise ValueError("num_envs, action_dim and nstep must be >= 1, guard_rows >= 0")
        if self.R < self.nstep + self.guard_rows + 2:
            raise ValueError(f"rows {self.R}: at least nstep + guard_rows + 2 = {self.nstep + self.guard_rows + 2}")
        if self.D:
            self._check_demo_rows(priority_alpha)
        dev, S = self.device, (self.R + self.D) * self.N
        # zeros, not empty: slots no add() has reached are compared as part of the ring (two runs of one loop, a run
        # against its restored copy), and what the allocator hands back depends on whatever ran in the process before
        whole = (torch.zeros((S, self.frame_bytes), dtype=torch.uint8, device=dev),
                 torch.zeros((S, self.A), dtype=torch.float32, device=dev),
                 torch.zeros((S,), dtype=torch.float32, device=dev),
                 torch.ones((S,), dtype=torch.float32, device=dev),
                 torch.ones((S,), dtype=torch.uint8, device=dev))
        # the ring is the first R N slots of each array, the partition the D N behind them; without demonstrations
        # the ring IS the allocation.  Everything that adds, exports or saves the ring works on these views
        live = self.R * self.N
        self.frames, self.action, self.reward, self.discount, self.first = (t[:live] if self.D else t for t in whole)
        self._whole = dict(zip(self._RING, whole))
        self._demo = {n: t[live:] for n, t in self._whole.items()}
        self.demo_rows_filled = 0   # Td: rows of the partition that add_demonstrations() has written
        self._demo_fraction = 0.0
        self.last_demo_count = 0    # Bd of the newest batch: its rows 0 .. Bd-1 are demonstrations
        self.T = 0                  # rows added
        self.rng = np.random.RandomState(seed)
        self.indexed = bool(indexed)
        self.last_steps = None      # int32 [B] on the device: the window length of every row of the newest batch
        self.last_index = None      # int64 [3][B] on the device: its obs, next_obs and transition slots
        self._stage = None          # pinned + device staging of one row, for host inputs
        self._bufs = {}
        self._frames_out = {}
        alpha = _priority_args(self, priority_alpha, priority_beta, priority_eps)
        if alpha is not None:
            if not self.indexed:
                raise ValueError("prioritized sampling on the ring yields indexed batches: indexed=True required")
            _priority_tree(self, S, alpha)

    # ---- storage -------------------------------------------------------------------------
    def bounds(self):
        """(lo, hi): the drawable rows; hi < lo while there are none"""
        return max(1, self.T - self.R + 1 + self.guard_rows), self.T - self.nstep

    MAX_INDEXED_UNITS = 2 ** 31 - 1     # the fused aug+conv1 launch names its source as the int 3 * slot + g, g = 0 .. 2

    def _check_demo_rows(self, priority_alpha):
        """the refusals of demo_rows != 0, each a ValueError that says why"""
        D, R, N = self.D, self.R, self.N
        if D < self.nstep + 2:
            raise ValueError(f"demo_rows {D}: at least nstep + 2 = {self.nstep + 2} (a reset row, one transition and "
                             "its window)")
        if 3 * (R + D) * N > self.MAX_INDEXED_UNITS:
            raise ValueError(f"demo_rows {D}: (rows + demo_rows) x num_envs = {(R + D) * N} slots; update() gathers an "
                             "indexed batch by the 32-bit index 3 * slot + g (the fused aug+conv1 launch), which reaches "
                             f"{self.MAX_INDEXED_UNITS // 3} slots")
        if priority_alpha is not None:
            raise ValueError("demo_rows with priority_alpha: the sum tree covers the ring only; prioritized mixed draws "
                             "are not built")

    @property
    def demo_fraction(self):
        """The share of every batch that is drawn from the demonstrations, read at every draw: of B rows the first
        Bd = int(B * demo_fraction + 0.5) are.  In [0, 1] (ValueError), and 0 for a store without demo_rows."""
        return self._demo_fraction

    @demo_fraction.setter
    def demo_fraction(self, value):
        f = float(value)
        if isinstance(value, bool) or not (0.0 <= f <= 1.0):
            raise ValueError(f"demo_fraction {value!r}: a float in [0, 1]")
        if f > 0.0 and not self.D:
            raise ValueError(f"demo_fraction {value!r}: this store has no demonstration partition (demo_rows=0)")
        self._demo_fraction = f

    def demo_bounds(self):
        """(lo, hi) = (1, Td - nstep): the drawable rows of the partition; hi < lo while there are none"""
        return 1, self.demo_rows_filled - self.nstep

    def demo_count(self, batch_size):
        """Bd: how many rows of a batch of batch_size come from the demonstrations at the present demo_fraction"""
        return int(int(batch_size) * self._demo_fraction + 0.5)

    def _batch(self, prioritized, idx, act, rew, disc):
        """the indexed batch of a draw whose slots are idx [3][B]; its frames are the whole allocation, `slots` the
        position slots of its transitions (idx[2]: what explore.KnnBonus looks up)"""
        batch = (_PrioritizedIndexed if prioritized else IndexedBatch)(self._whole["frames"], idx[0], act, rew, disc, idx[1])
        batch.slots = idx[2]
        return batch

    def __len__(self):
        """drawable transitions, reset rows included: rows x environments"""
        lo, hi = self.bounds()
        return max(0, hi - lo + 1) * self.N

    def _row(self, x, name, shapes, dtypes):
        """one argument of add() as a contiguous tensor of its storage type, checked; still where the caller has it"""
        t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        if not torch.is_tensor(t):
            raise ValueError(f"add(): {name} must be a numpy array or a tensor")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"add(): {name} of shape {shapes[0]} required, got {tuple(t.shape)}")
        if t.dtype not in dtypes:
            raise ValueError(f"add(): {name} must be {dtypes[0]}, got {t.dtype}")
        if t.device.type != "cpu" and t.device != _lib.device_index(self.device):
            raise ValueError(f"add(): {name} is on {t.device}, the store on {self.device}")
        if t.dtype != dtypes[0]:
            t = t.to(dtypes[0])     # float64 / bool of the same device: a cast, no wait
        return t.contiguous()

    def _staged(self, k, t):
        """a host tensor -> the device, through the pinned buffer of argument k: a blocking copy, like add_episode's"""
        if self._stage is None:
            N, A, fb, dev = self.N, self.A, self.frame_bytes, self.device
            mk = lambda shape, dt: (torch.empty(shape, dtype=dt).pin_memory(), torch.empty(shape, dtype=dt, device=dev))
            self._stage = [mk((N, fb), torch.uint8), mk((N, A), torch.float32), mk((N,), torch.float32),
                           mk((N,), torch.float32), mk((N,), torch.uint8)]
        pin, dv = self._stage[k]
        pin.copy_(t.reshape(pin.shape))
        dv.copy_(pin, non_blocking=False)
        return dv

    def add(self, obs, action, reward, discount, first=None):
        """One row for all N environments: obs uint8 [N, *obs_shape] (the observation after the step), action [N, A],
        reward and discount [N] or [N, 1] (float32; float64 is cast), first bool / uint8 [N] (True = this row is the reset
        row of a new episode: obs is its first observation, the other three are dummies; None = no environment was
        reset).  Row 0 is a reset row for every environment whatever `first` says.  Tensors on the store's device are
        handed to the launch as they are and nothing waits; numpy arrays and host tensors are staged with a blocking
        copy."""
        N = self.N
        args = [self._row(obs, "obs", [(N,) + self.slot_shape, (N, self.frame_bytes)], (torch.uint8,))]
        args += self._scalar_rows(action, reward, discount, first)
        self._write_row(args, self._staged, lambda src: launch(
            "drq_vec_add", ptr(self.frames), ptr(self.action), ptr(self.reward), ptr(self.discount), ptr(self.first),
            self.R, N, self.A, self.frame_bytes, self.T, *(ptr(t) for t in src), device=self.device))

    def _scalar_rows(self, action, reward, discount, first):
        """what every add takes besides the frames, checked like them"""
        N, f32 = self.N, (torch.float32, torch.float64)
        return [self._row(action, "action", [(N, self.A)], f32),
                self._row(reward, "reward", [(N,), (N, 1)], f32),
                self._row(discount, "discount", [(N,), (N, 1)], f32),
                None if first is None else self._row(first, "first", [(N,)], (torch.uint8, torch.bool))]

    def _write_row(self, args, staged, write):
        """the tail every add shares: host arguments are staged (staged(k, t): argument k on the device), write(src)
        launches the entry that writes row T, then the row counts and the tree follows"""
        N = self.N
        _on_gpu(self, "the step-major replay lives")
        with torch.cuda.device(self.device):
            src = [t if t is None or t.is_cuda else staged(k, t) for k, t in enumerate(args)]
            write(src)
            for t in src:           # a caller's tensor may be freed right after add(): the launch still reads it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
            self._row_added()

    def _row_added(self):
        """counts one written row and lets the tree follow (inside torch.cuda.device(self.device))"""
        self.T += 1
        if self.tree is not None:
            # hi and lo move by at most one row per add: the new hi enters (its flags were written nstep - 1 adds
            # ago, on this stream), the old lo leaves
            lo, hi = self.bounds()
            enter, leave = (hi if hi >= lo else -1), (lo - 1 if lo >= 2 else -1)
            if enter >= 0 or leave >= 0:
                launch("drq_vec_per_advance", ptr(self.tree), self.tree_leaves, ptr(self.first), self.R, self.N, self.T,
                       enter, leave, device=self.device)

    # ---- sampling ------------------------------------------------------------------------
    def sample(self, batch_size):
        """IndexedBatch (indexed=True: the frames stay in the ring) or the materialised 5-tuple of the reference's loader,
        shaped like DeviceReplay's.  One random_sample((B, K)) call on the store's RandomState per batch."""
        _on_gpu(self, "the step-major replay lives")
        lo, hi = self.bounds()
        B, K, dev = int(batch_size), self.K, self.device
        Bd = self.demo_count(B)
        if Bd > 0 and self.demo_bounds()[1] < 1:
            raise _lib.DrqError(f"replay: demo_fraction {self._demo_fraction} asks for {Bd} demonstration rows of {B}, "
                                f"the partition holds {self.demo_rows_filled} rows and no drawable one (nstep "
                                f"{self.nstep}): add_demonstrations() first")
        if hi < lo and Bd < B:      # a batch of demonstrations alone needs no live row: pure pre-training
            raise _lib.DrqError(f"replay: {self.T} rows added, no drawable row yet (nstep {self.nstep})")
        if self.tree is not None:
            return self._sample_prioritized(B, lo, hi)
        f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        idx, act, rew, disc, steps, u, host = _rotating(self._bufs, B, lambda: (
            torch.empty((3, B), dtype=torch.int64, device=dev), f(B, self.A), f(B, 1), f(B, 1),
            torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.float64, device=dev),
            torch.empty((B, K), dtype=torch.float64).pin_memory()))
        host.numpy()[:] = self.rng.random_sample((B, K))
        u.copy_(host, non_blocking=True)
        obs = nxt = None
        if not self.indexed:
            out = self._frames_out.get(B)
            if out is None:         # one batch size at a time, reused every call (DeviceReplay.gather's buffers)
                out = tuple(torch.empty((B, self.stack_bytes), dtype=torch.uint8, device=dev) for _ in range(2))
                self._frames_out = {B: out}
            obs, nxt = out
        copies = not self.indexed and self._draw_copies
        if Bd == 0:
            launch("drq_vec_sample", ptr(self.first), ptr(self.action), ptr(self.reward), ptr(self.discount), self.R,
                   self.N, self.A, self.frame_bytes, lo, hi, ptr(u), B, K, self.nstep, self.gamma, ptr(idx), ptr(act),
                   ptr(rew), ptr(disc), ptr(steps), ptr(self.frames) if copies else None, ptr(obs) if copies else None,
                   ptr(nxt) if copies else None, device=dev)
        else:
            # rows 0 .. Bd-1 from the partition, the others from the ring: the same u table, one launch
            w = self._whole
            launch("drq_vec_sample_mixed", ptr(w["first"]), ptr(w["action"]), ptr(w["reward"]), ptr(w["discount"]), self.R,
                   self.D, self.N, self.A, self.frame_bytes, lo, hi, self.demo_rows_filled, ptr(u), B, Bd, K, self.nstep,
                   self.gamma, ptr(idx), ptr(act), ptr(rew), ptr(disc), ptr(steps), ptr(w["frames"]) if copies else None,
                   ptr(obs) if copies else None, ptr(nxt) if copies else None, device=dev)
        self.last_steps, self.last_index, self.last_demo_count = steps, idx, Bd
        batch = self._batch(False, idx, act, rew, disc)
        if self.indexed:
            return batch
        if not copies:              # the ring holds no whole observation to copy: the batch gathers them
            return batch.materialize(self.obs_shape, (obs, nxt))
        shp = (B,) + self.obs_shape
        return obs.view(shp), act, rew, disc, nxt.view(shp)

    def _sample_prioritized(self, B, lo, hi):
        """One stratified draw on the device: u ~ U[0,1)^B from the store's RandomState (one random_sample call per
        batch) -> drq_vec_per_sample.  Returns a PrioritizedBatch that is an IndexedBatch."""
        dev = self.device
        f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        idx, act, rew, disc, steps, w, u, host = _rotating(self._pbufs, B, lambda: (
            torch.empty((3, B), dtype=torch.int64, device=dev), f(B, self.A), f(B, 1), f(B, 1),
            torch.empty((B,), dtype=torch.int32, device=dev), f(B), torch.empty((B,), dtype=torch.float64, device=dev),
            torch.empty((B,), dtype=torch.float64).pin_memory()))
        host.numpy()[:] = self.rng.random_sample(B)
        u.copy_(host, non_blocking=True)
        launch("drq_vec_per_sample", ptr(self.tree), self.tree_leaves, ptr(self.first), ptr(self.action),
               ptr(self.reward), ptr(self.discount), self.R, self.N, self.A, self.T, lo, hi, ptr(u), B, self.nstep,
               self.gamma, float(self.priority_beta), ptr(idx), ptr(act), ptr(rew), ptr(disc), ptr(steps), ptr(w),
               device=dev)
        self.last_steps, self.last_index = steps, idx
        return self._batch(True, idx, act, rew, disc)._per(self, idx[2], w)

    def _stamp_now(self):
        return self.T               # the number of rows the ring held at the draw

    def _update_priorities(self, batch, td_abs):
        if self.T - batch._stamp >= self.guard_rows:
            return                      # the batch's slots may hold other transitions: see PrioritizedBatch.update_priorities
        pos = batch._pos
        B = _td_rows(pos, td_abs)
        lo, hi = self.bounds()
        launch("drq_vec_per_update", ptr(self.tree), self.tree_leaves, ptr(self.first), self.R, self.N, self.T, lo, hi,
               ptr(pos), ptr(td_abs), B, self.priority_alpha, self.priority_eps, device=self.device)

    def __iter__(self):
        return BatchIterator(lambda: self.sample(self.batch_size), self)

    batch_size = 256

    # ---- checkpoints ---------------------------------------------------------------------
    _RING = ("frames", "action", "reward", "discount", "first")

    def _config(self):
        cfg = {"R": self.R, "N": self.N, "A": self.A, "slot_shape": tuple(self.slot_shape), "nstep": self.nstep,
               "gamma": self.gamma, "guard_rows": self.guard_rows, "indexed": self.indexed,
               "priority_alpha": self.priority_alpha, "priority_eps": self.priority_eps}
        if self.D:      # only then: the states of stores without demonstrations stay what they were, both ways
            cfg["demo_rows"] = self.D
        return cfg

    def state_dict(self, frames=True):
        """The store as a plain dict of CPU tensors and Python scalars: "format": 1, "kind" (the class), "config" (R, N, A,
        slot_shape, nstep, gamma, guard_rows, indexed, priority_alpha, priority_eps), T, priority_beta, the RandomState
        ("rng": get_state() with the key as an int64 tensor), the LIVE slots of frames, action, reward, discount and first
        -- slot (t mod R) N + e holds row t, so the first min(T, R) N -- and, prioritized, the whole tree (double
        [2 leaves]; tree[0] is the running maximum).  frames=False leaves the five ring arrays out (the caller keeps the
        ring some other way).  The ring goes through host memory whole: frame_bytes per live slot.  This SYNCHRONISES
        the store's device.  The rotating staging sets are not state.  A store with demo_rows adds "demo_rows" to the
        configuration and saves "demo_rows_filled", "demo_fraction" and "demos": the first Td N slots of the partition's
        five arrays under the ring's names (left out with frames=False); one without saves exactly the above."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        live = min(self.T, self.R) * self.N
        name, key, pos, has_gauss, cached = self.rng.get_state()
        sd = {"format": 1, "kind": type(self).__name__, "config": self._config(), "T": self.T,
              "priority_beta": self.priority_beta, "live_slots": live, "ring": bool(frames),
              "rng": (name, torch.from_numpy(key.astype(np.int64)), int(pos), int(has_gauss), float(cached))}
        if frames:
            for n in self._RING:
                sd[n] = host(getattr(self, n)[:live])
        if self.tree is not None:
            sd["tree"] = host(self.tree)
        if self.D:
            # demonstrations: Td, the fraction and -- with the ring -- the first Td N slots of the partition's arrays
            sd["demo_rows_filled"], sd["demo_fraction"] = self.demo_rows_filled, self._demo_fraction
            if frames:
                sd["demos"] = {n: host(self._demo[n][:self.demo_rows_filled * self.N]) for n in self._RING}
        return sd

    def load_state_dict(self, sd, frames=True):
        """Restores what state_dict() saved, into a fresh or a used store; ValueError, with NOTHING changed, for a wrong
        "format" / "kind" (the class counts), a configuration that differs from this store's (every differing field is
        named), arrays of another shape, or a dict saved with frames=False -- unless frames=False here says the caller
        means it: T, the generator and the tree are restored, the ring arrays stay as they are.  After a load the slots
        above the live ones hold what the constructor puts there, last_steps and last_index are None, and the staging
        sets are kept.  Works on a CPU store as well (no launch is involved)."""
        cfg = self._config()
        if not self.D and isinstance(sd, dict) and isinstance(sd.get("config"), dict) and "demo_rows" in sd["config"]:
            cfg["demo_rows"] = 0        # a state with demonstrations into a store without: named like any other field
        check_state(self, sd, cfg)
        T, live = sd.get("T"), sd.get("live_slots")
        if not isinstance(T, int) or T < 0 or live != min(T, self.R) * self.N:
            raise ValueError(f"{type(self).__name__}.load_state_dict(): T {T!r} and live_slots {live!r} do not fit a ring "
                             f"of {self.R} rows x {self.N}")
        if frames and not sd.get("ring"):
            raise ValueError(f"{type(self).__name__}.load_state_dict(): the state was saved with frames=False and holds no "
                             "ring; load_state_dict(sd, frames=False) restores the rest")
        want = {n: ((live,) + tuple(getattr(self, n).shape[1:]), getattr(self, n).dtype) for n in self._RING} if frames else {}
        if self.tree is not None:
            want["tree"] = self.tree
        check_state(self, sd, tensors=want)
        rng = sd.get("rng")
        if (not isinstance(rng, (tuple, list)) or len(rng) != 5 or not torch.is_tensor(rng[1]) or rng[1].numel() != 624
                or not 0 <= int(rng[2]) <= 624):
            raise ValueError(f"{type(self).__name__}.load_state_dict(): no RandomState in the saved state")
        if self.D:
            Td, fraction = sd.get("demo_rows_filled"), sd.get("demo_fraction")
            if (not isinstance(Td, int) or not 0 <= Td <= self.D or not isinstance(fraction, float)
                    or not 0.0 <= fraction <= 1.0):
                raise ValueError(f"{type(self).__name__}.load_state_dict(): demo_rows_filled {Td!r} and demo_fraction "
                                 f"{fraction!r} do not fit a partition of {self.D} rows")
            if frames:
                demos = sd.get("demos")
                if not isinstance(demos, dict):
                    raise ValueError(f"{type(self).__name__}.load_state_dict(): the state holds no demonstrations")
                check_state(self, {"format": sd["format"], "kind": sd["kind"], **{f"demos.{n}": demos.get(n) for n in self._RING}},
                            tensors={f"demos.{n}": ((Td * self.N,) + tuple(self._demo[n].shape[1:]), self._demo[n].dtype)
                                     for n in self._RING})
        if frames:
            for n in self._RING:
                getattr(self, n)[:live].copy_(sd[n])
            self.action[live:].zero_()
            self.reward[live:].zero_()
            self.discount[live:].fill_(1.0)
            self.first[live:].fill_(1)
            if self.D:
                filled, d = Td * self.N, self._demo
                for n in self._RING:
                    d[n][:filled].copy_(sd["demos"][n])
                d["frames"][filled:].zero_()
                d["action"][filled:].zero_()
                d["reward"][filled:].zero_()
                d["discount"][filled:].fill_(1.0)
                d["first"][filled:].fill_(1)
        if self.tree is not None:
            self.tree.copy_(sd["tree"])
        if self.D:
            self.demo_rows_filled, self._demo_fraction = Td, fraction
        self.T, self.priority_beta = T, float(sd["priority_beta"])
        self.rng.set_state((rng[0], rng[1].numpy().astype(np.uint32), int(rng[2]), int(rng[3]), float(rng[4])))
        self.last_steps = self.last_index = None

    # ---- episode files -------------------------------------------------------------------
    _stack = 1      # frames per observation that drq_vec_export_rows puts together (a slot holds the whole observation)

    def export_episodes(self, directory, start_row=None, include_open=False, min_length=1, chunk_bytes=256 << 20):
        """Writes the episodes the ring holds whole into `directory` as the reference's files, one
        `<timestamp>_<idx>_<len>.npz` each through replay_buffer.save_episode: observation uint8 [len + 1, *obs_shape],
        action float32 [len + 1, A], reward and discount float32 [len + 1, 1]; index 0 is the reset transition with the
        reference's dummies (action 0, reward 0, discount 1), whatever add() was handed on that row.  idx continues
        after the files already there.  What make_replay_loader() and add_episodes() read.

        This WAITS for the GPU: it synchronises the store's device, reads the `first` flags back once and plans on the
        host (drqv2_amd.episodes.plan_export: an episode is listed when its reset row is still in the ring and the
        next reset row of its environment has been added).  The steps are gathered chunk by chunk, at most chunk_bytes
        each, one launch per chunk (drq_vec_export_rows) into two pinned buffers used in turn, so the host compresses
        one chunk while the next is gathered and copied.  Compression (np.savez_compressed) dominates the run time.

        start_row: only episodes that ended on row start_row - 1 or later.  The report carries next_row = T: a loop that
        passes the previous report's next_row exports every closed episode exactly once, as long as it calls before an
        episode's reset row leaves the ring (such an episode is counted as `headless`, not written).  include_open also
        writes the episodes still running, cut where they are (a later call writes them again, longer); min_length
        skips shorter ones.  Returns an ExportReport.  The ring, its RandomState, its tree and T are untouched:
        state_dict() before and after is equal."""
        import replay_buffer as RB          # at call time: replay_buffer imports this module
        _on_gpu(self, "the step-major replay lives")
        torch.cuda.synchronize(self.device)
        plan = _episodes.plan_export(self.first.cpu().numpy(), self.T, self.R, self.N, start_row, include_open, min_length)
        table = _episodes.export_table(plan.episodes)
        M, A, sb, dev = int(table.shape[0]), self.A, self.stack_bytes, self.device
        directory = pathlib.Path(directory)
        directory.mkdir(parents=True, exist_ok=True)
        idx = max((i for _, i, _ in RB._episode_files(directory)), default=-1) + 1
        files = []
        if M:
            rows = int(max(1, min(M, int(chunk_bytes) // (sb + 4 * A + 20))))
            mk = lambda pin: [torch.empty(s, dtype=d, device=None if pin else dev, pin_memory=pin) for s, d in (
                ((rows, sb), torch.uint8), ((rows, A), torch.float32), ((rows,), torch.float32), ((rows,), torch.float32),
                ((rows, 3), torch.int32))]
            dv, pins, done = mk(False), [mk(True), mk(True)], [None, None]
            state = {"cur": 0, "arrays": None, "idx": idx}
            offsets = np.concatenate([[0], np.cumsum([n + 1 for _, _, n in plan.episodes])])

            def drain(k, m0, m):
                """chunk [m0, m0 + m) has arrived in pinned set k: its steps go to their episodes, full ones to disk"""
                done[k].synchronize()
                obs, act, rew, disc = (t.numpy() for t in pins[k][:4])
                pos = m0
                while pos < m0 + m:
                    j = state["cur"]
                    n = plan.episodes[j][2]
                    if state["arrays"] is None:
                        state["arrays"] = {"observation": np.empty((n + 1,) + self.obs_shape, np.uint8),
                                           "action": np.empty((n + 1, A), np.float32),
                                           "reward": np.empty((n + 1, 1), np.float32),
                                           "discount": np.empty((n + 1, 1), np.float32)}
                    a = pos - int(offsets[j])
                    b = min(int(offsets[j + 1]), m0 + m) - int(offsets[j])
                    s = slice(pos - m0, pos - m0 + b - a)
                    ep = state["arrays"]
                    ep["observation"][a:b] = obs[s].reshape((b - a,) + self.obs_shape)
                    ep["action"][a:b] = act[s]
                    ep["reward"][a:b, 0] = rew[s]
                    ep["discount"][a:b, 0] = disc[s]
                    pos += b - a
                    if b == n + 1:
                        ts = datetime.datetime.now().strftime("%Y%m%dT%H%M%S")
                        fn = directory / f"{ts}_{state['idx']}_{n}.npz"
                        RB.save_episode(ep, fn)
                        files.append(fn)
                        state["cur"], state["arrays"], state["idx"] = j + 1, None, state["idx"] + 1

            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream()
                prev = None
                for c, m0 in enumerate(range(0, M, rows)):
                    k, m = c & 1, min(rows, M - m0)
                    pin = pins[k]                   # free: the chunk it held was drained before the previous launch
                    pin[4].numpy()[:m] = table[m0:m0 + m]
                    dv[4][:m].copy_(pin[4][:m], non_blocking=True)
                    launch("drq_vec_export_rows", ptr(self.frames), ptr(self.action), ptr(self.reward),
                           ptr(self.discount), self.R, self.N, A, self.frame_bytes, self._stack, ptr(dv[4]), m,
                           ptr(dv[0]), ptr(dv[1]), ptr(dv[2]), ptr(dv[3]), device=dev)
                    for q in range(4):
                        pin[q][:m].copy_(dv[q][:m], non_blocking=True)
                    done[k] = torch.cuda.Event()
                    done[k].record(stream)
                    if prev is not None:
                        drain(*prev)
                    prev = (k, m0, m)
                drain(*prev)
        return ExportReport(files, len(plan.episodes), sum(n for _, _, n in plan.episodes), plan.next_row,
                            plan.zero_length, plan.headless, plan.open, plan.short)

    def _episode_frames(self, obs, check):
        """what the slots of an episode hold: its `observation`, checked against the store (ValueError).  `check` is
        add_episodes()' argument: a slot holds the whole observation here, so there is no stack to verify and it is
        not read; VecFrameReplay's version does"""
        obs = np.asarray(obs)
        if obs.dtype != np.uint8 or obs.ndim < 1 or tuple(obs.shape[1:]) != self.slot_shape:
            raise ValueError(f"uint8 [len + 1, {', '.join(map(str, self.slot_shape))}] required, got {obs.dtype} "
                             f"{list(obs.shape)}")
        return np.ascontiguousarray(obs)

    def _checked_episode(self, ep, name, check, what="add_episodes()"):
        """an episode dict as planned_rows takes it, every field checked against the store: ValueError naming both"""
        def bad(field, why):
            return ValueError(f"{what}: {name}: {field}: {why}")
        for field in ("observation", "action", "reward", "discount"):
            if field not in ep:
                raise bad(field, "the episode has no such field")
        try:
            frame = self._episode_frames(ep["observation"], check)
        except ValueError as e:
            raise bad("observation", str(e)) from None
        n = frame.shape[0]
        if n < 2:
            raise bad("observation", f"{n} step(s): an episode needs its reset step and at least one transition")
        out = {"frame": frame}
        for field, shapes in (("action", [(n, self.A)]), ("reward", [(n,), (n, 1)]), ("discount", [(n,), (n, 1)])):
            x = np.asarray(ep[field])
            if x.dtype != np.float32:
                raise bad(field, f"float32 required, got {x.dtype}")
            if tuple(x.shape) not in shapes:
                raise bad(field, f"shape {list(shapes[0])} required (len + 1 = {n}, the store's action_dim = {self.A}), "
                                 f"got {list(x.shape)}")
            out[field] = np.ascontiguousarray(x)
        return out

    def add_episodes(self, source, check=True, chunk_bytes=256 << 20):
        """Fills the ring from episodes that already exist.  source: a directory of the reference's episode files (read
        with replay_buffer's own listing and load_episode, oldest first), or a list of episode dicts with `observation`
        uint8 [len + 1, *obs_shape], `action` float32 [len + 1, A], `reward` and `discount` float32 [len + 1] or
        [len + 1, 1].  All of them are held in host memory while the call runs.

        Every episode is checked against the store before anything is written: ValueError names the episode and the
        field.  drqv2_amd.episodes.plan_fill then lays them out as lockstep rows -- each episode, in order, into the
        environment with the fewest rows so far, the shorter environments padded at their end with reset rows -- and if
        that takes L > R rows per environment it is a ValueError too: split the data or enlarge the ring.  The rows are
        staged step-major through two pinned buffers used in turn, at most chunk_bytes each, and written with one launch
        per chunk (drq_vec_fill); a prioritized store's tree then follows row by row (drq_vec_per_advance), as after
        add().  The store ends in the state L add() calls with the planned rows (drqv2_amd.episodes.planned_rows) would
        have left, bit for bit: frames, action, reward, discount, first, T and the tree.  Checkpoints need nothing new.

        A look-ahead batch drawn before the call is stale, as after any `guard_rows` adds: make a new iterator.  Every
        environment ends on a finished episode (or a pad row), so the next live add() must be a reset row for every
        environment.  Returns a FillReport.  DrqError for a store on the CPU, after the checks."""
        eps, lengths, plan = self._planned_episodes(source, check, "add_episodes()")
        L, R = plan.L, self.R
        if L > R:
            raise ValueError(f"add_episodes(): {len(eps)} episodes need L = {L} rows per environment, the ring has R = {R}: "
                             "split the data or enlarge the ring")
        _on_gpu(self, "the step-major replay lives")
        report = FillReport(len(eps), sum(lengths), L, plan.pad_rows)
        if L == 0:
            return report
        # a prioritized store: no row of a chunk may overwrite flags the tree still has to read for an earlier row of
        # it (the row that enters is nstep - 1 rows behind the one just written)
        cap = R - self.nstep if self.tree is not None else R

        def rows_added(n):
            for _ in range(n):
                self._row_added()
        self._fill_rows(plan, eps, cap, chunk_bytes, [getattr(self, n) for n in self._RING], R, lambda: self.T, rows_added)
        return report

    def _planned_episodes(self, source, check, what):
        """(episodes, lengths, plan): what add_episodes() and add_demonstrations() take -- a directory of episode files
        or episode dicts -- read, every episode checked against the store, and laid out as lockstep rows"""
        import replay_buffer as RB          # at call time: replay_buffer imports this module
        if isinstance(source, (str, pathlib.Path)):
            files = [fn for fn, _, _ in RB._episode_files(source)]
            named = [(fn.name, RB.load_episode(fn)) for fn in files]
        else:
            named = [(f"episode {i}", ep) for i, ep in enumerate(source)]
        eps = [self._checked_episode(ep, name, check, what) for name, ep in named]
        lengths = [ep["frame"].shape[0] - 1 for ep in eps]
        return eps, lengths, _episodes.plan_fill(lengths, self.N)

    def _fill_rows(self, plan, eps, cap, chunk_bytes, arrays, R, row_of, rows_added):
        """The plan's L rows staged step-major through two pinned buffers used in turn, at most chunk_bytes and `cap` rows
        a chunk, each written by one drq_vec_fill into `arrays` (frames, action, reward, discount, first of R rows) from
        row row_of() on; rows_added(n) counts the n rows of a chunk."""
        L, N, A, dev = plan.L, self.N, self.A, self.device
        rows = int(max(1, min(L, cap, int(chunk_bytes) // (N * (self.frame_bytes + 4 * A + 9)))))
        mk = lambda pin: [torch.empty(s, dtype=d, device=None if pin else dev, pin_memory=pin) for s, d in (
            ((rows, N) + self.slot_shape, torch.uint8), ((rows, N, A), torch.float32), ((rows, N), torch.float32),
            ((rows, N), torch.float32), ((rows, N), torch.uint8))]
        dv, pins, done = mk(False), [mk(True), mk(True)], [None, None]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream()
            for c, r0 in enumerate(range(0, L, rows)):
                k, n = c & 1, min(rows, L - r0)
                if done[k] is not None:
                    done[k].synchronize()       # the upload of the chunk this pinned set held has run
                _episodes.planned_rows(plan, eps, r0, r0 + n, out=[t.numpy() for t in pins[k]])
                for d, p in zip(dv, pins[k]):
                    d[:n].copy_(p[:n], non_blocking=True)
                done[k] = torch.cuda.Event()
                done[k].record(stream)
                launch("drq_vec_fill", *(ptr(t) for t in arrays), R, N, A, self.frame_bytes, row_of(), n,
                       *(ptr(d) for d in dv), device=dev)
                rows_added(n)
            for ev in done:
                if ev is not None:
                    ev.synchronize()

    # ---- demonstrations ------------------------------------------------------------------
    def add_demonstrations(self, source, check=True, chunk_bytes=256 << 20):
        """Appends episodes to the demonstration partition (demo_rows > 0).  source, check and chunk_bytes are
        add_episodes()': a directory of the reference's episode files or a list of episode dicts, every episode checked
        against the store before anything is written (ValueError names the episode and the field), laid out as lockstep
        rows by drqv2_amd.episodes.plan_fill -- each episode into the lane with the fewest rows, the shorter lanes padded
        with reset rows -- and written by drq_vec_fill, called on the partition's base pointers with R = demo_rows, one
        launch per staging chunk.  The L rows go behind the Td = demo_rows_filled rows already there and hold
        drqv2_amd.episodes.planned_rows(plan, episodes, 0, L), bit for bit.  The partition never evicts:
        Td + L > demo_rows is a ValueError before anything is written.  The ring, T and the RandomState are untouched,
        and a batch drawn earlier stays valid: rows that were drawable are never written again.  Returns a FillReport
        (rows = L; T does not grow).  DrqError for a store on the CPU, after the checks."""
        if not self.D:
            raise ValueError("add_demonstrations(): this store has no demonstration partition (demo_rows=0)")
        eps, lengths, plan = self._planned_episodes(source, check, "add_demonstrations()")
        L, D, Td = plan.L, self.D, self.demo_rows_filled
        if Td + L > D:
            raise ValueError(f"add_demonstrations(): {len(eps)} episodes need L = {L} rows per lane behind the {Td} already "
                             f"filled, the partition has demo_rows = {D} and never evicts: enlarge it or pass fewer episodes")
        _on_gpu(self, "the step-major replay lives")
        report = FillReport(len(eps), sum(lengths), L, plan.pad_rows)
        if L == 0:
            return report

        def rows_added(n):
            self.demo_rows_filled += n
        self._fill_rows(plan, eps, D, chunk_bytes, [self._demo[n] for n in self._RING], D, lambda: self.demo_rows_filled,
                        rows_added)
        return report


class VecFrameReplay(VecDeviceReplay):
    """VecDeviceReplay with ONE frame per slot (new; the contract is in include/drqv2_hip.h, "single-frame step-major
    replay"): add() takes the newest uint8 [N, 3, 84, 84] frame of every environment, as a renderer hands it out, and a
    slot is 21,168 bytes instead of the 63,504 of a three-frame stack whose two older frames its neighbours hold anyway.
    The 9-channel observation is put together when it is read, by the rule of the reference's FrameStackWrapper
    (dmc.py:87-109): the frames of rows t-2, t-1, t of the environment, refilled with the episode's first frame where a
    reset row lies among them.  Nobody stacks on the host:
      observation()   the stacks of the newest row, for agent.act_batch()
      sample()        a FrameBatch (indexed=True): the frames stay in the ring, update()'s fused aug+conv1 launch
                      gathers the stacks itself; indexed=False: the materialised 5-tuple, gathered by one kernel
    and nobody resizes or transposes in front of add(): add_render() takes the renderer's own uint8 [N, S, S, 3 or 4]
    image, S = 84 .. 336, and writes the frames with one launch by an exact integer area average.
    Everything else -- rows, flags, windows, draws, `priority_alpha`, guard_rows -- is VecDeviceReplay's, launch for
    launch.  The drawable rows start two rows later, lo = max(1, T - rows + 1 + guard_rows + 2): the oldest frame of an
    obs stack lies three rows before its transition and must stay in the ring while guard_rows rows are added; hence
    rows >= nstep + guard_rows + 4.  A VecDeviceReplay(guard_rows + 2) fed the stacks draws the same batches.
    Restrictions of update() on these batches: single GPU, no behaviour cloning, and prioritized batches in fp32 only.
    Only three-frame stacks of 3 x 84 x 84 frames: the kernels that gather are built for them."""

    _draw_copies = False
    _stack = 3              # export_episodes() writes the 9-channel stacks, put together by the launch that gathers them

    def _episode_frames(self, obs, check):
        """add_episodes() takes uint8 [len + 1, 9, 84, 84] frame stacks and keeps the newest frame of each -- check: after
        verifying that they are what a FrameStackWrapper builds (newest_frames) -- or [len + 1, 3, 84, 84] single frames
        as they are"""
        return newest_frames(obs, check)

    def __init__(self, rows, num_envs, action_dim, nstep, discount, device, frame_shape=(3, 84, 84), seed=None,
                 indexed=True, guard_rows=8, priority_alpha=None, priority_beta=0.4, priority_eps=1e-6, demo_rows=0):
        if tuple(int(s) for s in frame_shape) != (3, 84, 84):
            raise ValueError(f"frame_shape {tuple(frame_shape)}: the single-frame ring stacks three (3, 84, 84) frames")
        if int(demo_rows):
            raise ValueError(f"demo_rows {demo_rows}: a single-frame ring holds no demonstrations -- its stacks are put "
                             "together modulo the ring's rows, which a partition behind them is not part of; use "
                             "VecDeviceReplay")
        if int(rows) < int(nstep) + int(guard_rows) + 4:
            raise ValueError(f"rows {rows}: at least nstep + guard_rows + 4 = {int(nstep) + int(guard_rows) + 4}")
        super().__init__(rows, num_envs, frame_shape, action_dim, nstep, discount, device, seed=seed, indexed=indexed,
                         guard_rows=guard_rows, priority_alpha=priority_alpha, priority_beta=priority_beta,
                         priority_eps=priority_eps)
        self.frame_shape = self.slot_shape
        self.obs_shape = (9, 84, 84)               # what observation() and a materialised batch hold
        self.stack_bytes = 3 * self.frame_bytes
        self._obs_out = None
        self._render_stage = None   # pinned + device staging of one host image of add_render()

    def bounds(self):
        """(lo, hi): the drawable rows; hi < lo while there are none"""
        return max(1, self.T - self.R + 1 + self.guard_rows + 2), self.T - self.nstep

    def _batch(self, prioritized, idx, act, rew, disc):
        batch = (_PrioritizedFrames if prioritized else FrameBatch)(self.frames, idx[0], act, rew, disc, idx[1], self.first,
                                                                    self.R, self.N)
        batch.slots = idx[2]
        return batch

    def add(self, frame, action, reward, discount, first=None):
        """As VecDeviceReplay.add(), with frame uint8 [N, 3, 84, 84]: the newest frame of every environment after the
        step (on a reset row: the first frame of the new episode)."""
        super().add(frame, action, reward, discount, first)

    RENDER_SIZES = (84, 336)    # no upsampling; 4 x 84: at most 5 taps per axis, sums < 2^31, 41 KB of LDS per band

    def _image(self, x):
        """the image of add_render() as a contiguous uint8 tensor, checked; still where the caller has it"""
        t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        lo, hi = self.RENDER_SIZES
        if not torch.is_tensor(t):
            raise ValueError("add_render(): image must be a numpy array or a tensor")
        if t.dim() != 4 or t.shape[0] != self.N:
            raise ValueError(f"add_render(): image of shape ({self.N}, S, S, 3 or 4) required, got {tuple(t.shape)}")
        if t.shape[1] != t.shape[2]:
            raise ValueError(f"add_render(): image must be square, got {t.shape[1]} x {t.shape[2]}")
        if not lo <= t.shape[1] <= hi:
            raise ValueError(f"add_render(): image size {lo} .. {hi} required, got {t.shape[1]}")
        if t.shape[3] not in (3, 4):
            raise ValueError(f"add_render(): image with 3 or 4 channels last required, got {t.shape[3]}")
        if t.dtype != torch.uint8:
            raise ValueError(f"add_render(): image must be {torch.uint8}, got {t.dtype}")
        if t.device.type != "cpu" and t.device != _lib.device_index(self.device):
            raise ValueError(f"add_render(): image is on {t.device}, the store on {self.device}")
        t = t.contiguous()
        return t.clone() if t.data_ptr() % 4 else t        # a view that starts inside a dword: the kernel reads dwords

    def _staged_image(self, t):
        """a host image -> the device, through a pinned buffer of its shape: a blocking copy, like _staged()"""
        if self._render_stage is None or self._render_stage[0].shape != t.shape:
            self._render_stage = (torch.empty(t.shape, dtype=torch.uint8).pin_memory(),
                                  torch.empty(t.shape, dtype=torch.uint8, device=self.device))
        pin, dv = self._render_stage
        pin.copy_(t)
        dv.copy_(pin, non_blocking=False)
        return dv

    def add_render(self, image, action, reward, discount, first=None):
        """add() for the image a renderer hands out: uint8 [N, S, S, 3 or 4], channels last, S = 84 .. 336 (a fourth
        channel is never read).  One launch (drq_vec_add_render) resizes it to the [N, 3, 84, 84] frames of the row by
        the exact integer area average of include/drqv2_hip.h, "renderer images" -- S = 84: the transposition, S = 84 k:
        the mean of every k x k block rounded half up -- and writes action, reward, discount and first as add() does.
        The effect is add(resize(image), ...), bit for bit; the other arguments, their checks and what follows the
        launch are add()'s, and the two may alternate on one store.  An image on the store's device goes to the
        launch as it is; a numpy array or host tensor is staged through a pinned buffer of its shape with a blocking
        copy."""
        args = [self._image(image)] + self._scalar_rows(action, reward, discount, first)
        S, Cin = int(args[0].shape[1]), int(args[0].shape[3])
        self._write_row(args, lambda k, t: self._staged_image(t) if k == 0 else self._staged(k, t),
                        lambda src: launch("drq_vec_add_render", ptr(self.frames), ptr(self.action), ptr(self.reward),
                                           ptr(self.discount), ptr(self.first), self.R, self.N, self.A, self.T,
                                           ptr(src[0]), S, Cin, *(ptr(t) for t in src[1:]), device=self.device))

    def observation(self):
        """uint8 [N, 9, 84, 84] on the device: the frame stacks of the newest row, what a FrameStackWrapper per
        environment would return after the last add() -- ready for agent.act_batch().  One launch
        (drq_vec_stack_gather), nothing waits.  Two output buffers are used in turn: a returned tensor is overwritten
        by the second observation() call after it, so a caller that keeps one longer clones it."""
        _on_gpu(self, "the step-major replay lives")
        if self.T == 0:
            raise _lib.DrqError("observation(): no row has been added yet")
        if self._obs_out is None:
            self._obs_out = [torch.empty((self.N,) + self.obs_shape, dtype=torch.uint8, device=self.device)
                             for _ in range(2)] + [0]
        out = self._obs_out[self._obs_out[2]]
        self._obs_out[2] ^= 1
        launch("drq_vec_stack_gather", ptr(self.frames), ptr(self.first), self.R, self.N, self.frame_bytes, None,
               self.T - 1, self.N, ptr(out), device=self.device)
        return out


class EpisodeSnapshot:
    """What VecEpisodeStats.poll() / read() return: a copy of one host mirror, so it stays what it is.
      rows, episodes, length_sum, return_sum, min_return, max_return   the header (include/drqv2_hip.h, "episode statistics")
      mean_return, mean_length   return_sum / episodes, length_sum / episodes; nan while episodes == 0
      complete   max_episodes_per_env = k > 0: episodes == k * num_envs (every environment has finished its k); else False
      records    numpy structured array (return f32, length i32, env i32, row i64): the newest min(episodes, log_size)
                 counted episodes, oldest first -- the order (row, env)
      lost       max(0, episodes - log_size): the episodes the log no longer holds
      seq        the number of the publish() that produced it"""

    RECORD = np.dtype([("return", np.float32), ("length", np.int32), ("env", np.int32), ("row", np.int64)])

    def __init__(self, raw, W, N, limit, seq):
        """raw: uint8 array, the mirror's bytes in the layout of drq_vec_stats_publish"""
        raw = np.array(raw, copy=True)
        i64, f32 = raw[:24].view(np.int64), raw[32:40].view(np.float32)
        self.rows, self.episodes, self.length_sum = int(i64[0]), int(i64[1]), int(i64[2])
        self.return_sum = float(raw[24:32].view(np.float64)[0])
        self.min_return, self.max_return = float(f32[0]), float(f32[1])
        self.seq, self.log_size = int(seq), int(W)
        n = min(self.episodes, W)
        at = np.arange(self.episodes - n, self.episodes, dtype=np.int64) % W       # oldest first
        rec = np.empty(n, self.RECORD)
        rec["return"] = raw[64:64 + 4 * W].view(np.float32)[at]
        rec["length"] = raw[64 + 4 * W:64 + 8 * W].view(np.int32)[at]
        rec["env"] = raw[64 + 8 * W:64 + 12 * W].view(np.int32)[at]
        row0 = _stats_row_offset(W)
        rec["row"] = raw[row0:row0 + 8 * W].view(np.int64)[at]
        self.records = rec
        self.lost = max(0, self.episodes - W)
        self.complete = limit > 0 and self.episodes == limit * N
        nan = float("nan")
        self.mean_return = self.return_sum / self.episodes if self.episodes else nan
        self.mean_length = self.length_sum / self.episodes if self.episodes else nan

    def since(self, prev_episodes):
        """(records, missed): the counted episodes with global number >= prev_episodes (the `episodes` of the snapshot
        the caller logged last) that are still in the log, oldest first, and how many of them the log has lost"""
        prev = max(0, int(prev_episodes))
        oldest = self.episodes - len(self.records)
        return self.records[max(0, prev - oldest):], max(0, oldest - prev)

    def __repr__(self):
        return (f"EpisodeSnapshot(rows={self.rows}, episodes={self.episodes}, mean_return={self.mean_return:.6g}, "
                f"mean_length={self.mean_length:.6g}, min_return={self.min_return:.6g}, max_return={self.max_return:.6g}, "
                f"lost={self.lost}, complete={self.complete})")


def _stats_row_offset(W):
    """byte offset of the int64 rows in a mirror of drq_vec_stats_publish: behind the three 4-byte arrays, 8-byte aligned"""
    return (64 + 12 * W + 7) & ~7


class VecEpisodeStats:
    """Episode returns and lengths of N lockstep environments, kept on the device (new; the contract is in
    include/drqv2_hip.h, "episode statistics").  It is fed the `reward` and `first` tensors the caller already hands to
    VecDeviceReplay.add() / VecFrameReplay.add(), but knows no store, so an evaluation loop uses it as well:

        stats = VecEpisodeStats(num_envs=N, device="cuda")
        ...
        store.add(frame, action, reward, discount, first)
        stats.step(reward, first)           # one launch (drq_vec_stats_step), nothing waits
        if step % 1000 == 0:
            stats.publish()                 # one launch: the state -> a pinned host mirror; nothing waits
            snap = stats.poll()             # the newest EpisodeSnapshot that has ARRIVED, or None; never waits

    Call 0 is a reset row for every environment, like row 0 of the ring.  A `first` flag on a later call closes the
    running episode of its environment -- unless that is empty (two resets in a row) -- as a record (return, length, env,
    row) in a log of the newest `log_size` episodes and in the totals; the reward of a reset row is a dummy and is not
    read; every other reward is added to the running return with one float32 add (the reference's
    `episode_reward += time_step.reward`, train.py:186).  max_episodes_per_env = k > 0 (evaluation) counts the first k
    episodes of EVERY environment and nothing after them -- "until K episodes have finished" would favour short ones --
    and `snapshot.complete` says when all have theirs.
    publish() uses FOUR pinned mirrors in turn (the idea of _rotating) and numbers them 1, 2, ...: poll() returns a
    snapshot of the newest mirror whose sequence word equals the number it was published with.  read() publishes and
    waits for that one.  episode_return / episode_length are the running device tensors, read-only by convention."""

    _row = VecDeviceReplay._row      # add()'s checks and messages

    def __init__(self, num_envs, device, log_size=1024, max_episodes_per_env=0):
        self.N, self.W, self.limit = int(num_envs), int(log_size), int(max_episodes_per_env)
        if self.N < 1 or self.W < 1 or self.limit < 0:
            raise ValueError("num_envs and log_size must be >= 1, max_episodes_per_env >= 0")
        self.device = dev = torch.device(device)
        N, W = self.N, self.W
        self.episode_return = torch.zeros(N, dtype=torch.float32, device=dev)
        self.episode_length = torch.zeros(N, dtype=torch.int32, device=dev)
        self.episodes_done = torch.zeros(N, dtype=torch.int32, device=dev)
        self.header = torch.zeros(8, dtype=torch.int64, device=dev)
        self._log = (torch.zeros(W, dtype=torch.float32, device=dev), torch.zeros(W, dtype=torch.int32, device=dev),
                     torch.zeros(W, dtype=torch.int32, device=dev), torch.zeros(W, dtype=torch.int64, device=dev))
        self.rows = 0               # step() calls so far: the row number of the next one
        self.published = 0          # publish() calls so far: the sequence number of the newest
        self._stage = None          # pinned + device staging of reward and first, for host inputs
        self._seq_at = _stats_row_offset(W) + 8 * W
        self._mirrors = None        # four of [pinned uint8 tensor, its numpy view, its sequence word, the number expected]
        if dev.type == "cuda":
            self._launch_reset()

    def _state(self):
        return [ptr(self.episode_return), ptr(self.episode_length), ptr(self.episodes_done), ptr(self.header)] + \
            [ptr(t) for t in self._log]

    def _launch_reset(self):
        launch("drq_vec_stats_reset", *self._state(), self.N, self.W, device=self.device)

    def _staged(self, k, t):
        if self._stage is None:
            mk = lambda dt: (torch.empty(self.N, dtype=dt).pin_memory(), torch.empty(self.N, dtype=dt, device=self.device))
            self._stage = [mk(torch.float32), mk(torch.uint8)]
        pin, dv = self._stage[k]
        pin.copy_(t.reshape(pin.shape))
        dv.copy_(pin, non_blocking=False)
        return dv

    def step(self, reward, first=None):
        """reward float32 [N] or [N, 1] (float64 is cast), first bool / uint8 [N] or None = no environment was reset:
        the tensors of the store's add(), checked by the same rules.  Tensors on the device go to the launch as they are
        and nothing waits; numpy arrays and host tensors are staged with a blocking copy."""
        N = self.N
        args = [self._row(reward, "reward", [(N,), (N, 1)], (torch.float32, torch.float64)),
                None if first is None else self._row(first, "first", [(N,)], (torch.uint8, torch.bool))]
        _on_gpu(self, "the episode statistics live")
        with torch.cuda.device(self.device):
            src = [t if t is None or t.is_cuda else self._staged(k, t) for k, t in enumerate(args)]
            launch("drq_vec_stats_step", *self._state(), N, self.W, self.limit, self.rows, ptr(src[0]), ptr(src[1]),
                   device=self.device)
            for t in src:           # a caller's tensor may be freed right after step(): the launch still reads it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
            self.rows += 1

    def reset(self):
        """One launch puts everything back to the initial state (one object serves many evaluations): the next step()
        is a reset row again.  Snapshots published before stay readable; the sequence numbers go on."""
        _on_gpu(self, "the episode statistics live")
        self._launch_reset()
        self.rows = 0

    def publish(self):
        """One launch (drq_vec_stats_publish) copies the state, as it is after every step() enqueued so far, into the next
        of the four pinned mirrors; nothing waits.  Returns the sequence number of this publish."""
        _on_gpu(self, "the episode statistics live")
        if self._mirrors is None:
            self._mirrors = []
            for _ in range(4):
                pin = torch.zeros(self._seq_at + 8, dtype=torch.uint8).pin_memory()
                view = pin.numpy()
                self._mirrors.append([pin, view, view[self._seq_at:self._seq_at + 4].view(np.uint32), None])
        self.published += 1
        m = self._mirrors[(self.published - 1) & 3]
        m[3] = self.published & 0xFFFFFFFF
        launch("drq_vec_stats_publish", ptr(self.header), *(ptr(t) for t in self._log), self.W, ptr(m[0]), m[3],
               device=self.device)
        return self.published

    def _snapshot(self, m):
        return EpisodeSnapshot(m[1], self.W, self.N, self.limit, m[3])

    # ---- checkpoints ---------------------------------------------------------------------
    _LOG = ("log_return", "log_length", "log_env", "log_row")

    def _tensors(self):
        t = {k: getattr(self, k) for k in ("episode_return", "episode_length", "episodes_done", "header")}
        t.update(zip(self._LOG, self._log))
        return t

    def state_dict(self):
        """The statistics as a plain dict of CPU tensors and Python scalars: "format": 1, "kind", "config" (N, W, limit),
        episode_return, episode_length, episodes_done, header, the four log arrays and rows.  The publish sequence number
        and the pinned mirrors belong to the live object.  This SYNCHRONISES the object's device."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        sd = {"format": 1, "kind": type(self).__name__, "config": {"N": self.N, "W": self.W, "limit": self.limit},
              "rows": self.rows}
        sd.update((k, host(t)) for k, t in self._tensors().items())
        return sd

    def load_state_dict(self, sd):
        """Restores what state_dict() saved, into a fresh or a used object; ValueError, with nothing changed, for a wrong
        "format" / "kind" or a configuration that differs (every differing field is named).  The sequence numbers of
        publish() simply go on; a read() after the load returns the header and records of a read() before the save."""
        check_state(self, sd, {"N": self.N, "W": self.W, "limit": self.limit}, self._tensors())
        if not isinstance(sd.get("rows"), int) or sd["rows"] < 0:
            raise ValueError(f"VecEpisodeStats.load_state_dict(): rows {sd.get('rows')!r}")
        for k, t in self._tensors().items():
            t.copy_(sd[k])
        self.rows = sd["rows"]

    def poll(self):
        """The EpisodeSnapshot of the newest publish() that has arrived on the host, or None if none has.  Never waits
        and never synchronises: it compares four sequence words."""
        for back in range(min(4, self.published)):
            m = self._mirrors[(self.published - 1 - back) & 3]
            if int(m[2][0]) == m[3]:
                return self._snapshot(m)
        return None

    def read(self, timeout=30.0):
        """publish(), then wait for it: short sleeps until its sequence word shows; DrqError after `timeout` seconds
        (and one synchronise of this object's device)."""
        import time
        self.publish()
        m = self._mirrors[(self.published - 1) & 3]
        t0 = time.perf_counter()
        while int(m[2][0]) != m[3]:
            if time.perf_counter() - t0 > timeout:
                torch.cuda.synchronize(self.device)
                if int(m[2][0]) != m[3]:
                    raise _lib.DrqError(f"VecEpisodeStats.read(): publish {self.published} has not arrived after {timeout} s")
                break
            time.sleep(20e-6)
        return self._snapshot(m)
