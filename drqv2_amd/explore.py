"""Count-based exploration bonus for vectorised collection (new; the reference explores by the noise of its policy alone,
drqv2.py:164-175, and every reward its replay sees is the environment's own).

SimHashBonus is the bonus of "#Exploration" (Tang et al. 2017) on the frames of N lockstep environments where they
already are: a SimHash of every frame (a 21 x 21 grid of block sums, centred, `bits` random +-1 projections, their signs),
a table of 2^bits visit counts in HBM, bonus = beta / sqrt(count).  One call is two launches on the current stream
(csrc/explore.hip, drq_explore_simhash_step) and no host wait; the contract is spelled out to the bit in
include/drqv2_hip.h ("exploration bonus") and restated in numpy by tests/simhash_oracle.py.
"""
import math

import torch

from . import _lib
from ._lib import launch, ptr
from .checkpoint import check_state, host


MAX_BITS = 24        # DRQ_SIMHASH_MAX_BITS


class SimHashBonus:
    """
        bonus = SimHashBonus(num_envs=N, device="cuda", bits=16, beta=0.1, seed=0)
        r = bonus.step(frame, reward)            # reward + bonus, float32 [N] on the device
        b = bonus.step(frame)                    # the bonus alone
        b = bonus.step(frame, update=False)      # look up without counting (evaluation, diagnostics)

    frame is what the device environments return and VecFrameReplay.add() takes: uint8 [N, 3, 84, 84] on this object's
    device.  A counting step first adds 1 to the count of every environment's code and then reads the counts, so two
    environments with the same code in one step both get the count after both increments; a step with update=False
    changes nothing, and the bonus of a code never counted is beta.  codes and counts are the int32 [N] tensors of the
    newest step, last_bonus its float32 [N] bonus (whether or not a reward was given).

    Every return is a device tensor written by launches on the current stream; nothing waits for the GPU.  step()
    writes into TWO output sets (codes, counts, bonus, reward + bonus) used in turn, as the device environments and
    VecFrameReplay.observation() do: a returned tensor is overwritten by the second step() call after it, so a caller
    that keeps one longer clones it.

    distinct() is the number of codes counted so far, reset() empties the table; state_dict() / load_state_dict() keep
    the table in sparse form and go into a checkpoint through checkpoint.save(..., bonus=bonus)."""

    FRAME_SHAPE = (3, 84, 84)

    def __init__(self, num_envs, device, bits=16, beta=0.1, seed=0):
        if isinstance(bits, bool) or not isinstance(bits, int) or not 1 <= bits <= MAX_BITS:
            raise ValueError(f"bits must be an int in 1 .. {MAX_BITS}, got {bits!r}")
        self.N, self.bits, self.beta = int(num_envs), bits, float(beta)
        if self.N < 1:
            raise ValueError("num_envs must be >= 1")
        if not math.isfinite(self.beta) or self.beta < 0:
            raise ValueError(f"beta must be a finite number >= 0, got {beta!r}")
        self.seed = int(seed) & 0xFFFFFFFF
        self.device = torch.device(device)
        self.table = torch.zeros(1 << bits, dtype=torch.int32, device=self.device)
        self.codes = self.counts = self.last_bonus = None      # of the newest step()
        self._out = None            # two of (codes, counts, bonus, reward + bonus), then the index of the next

    def _on_gpu(self):
        if self.device.type != "cuda":
            raise _lib.DrqError("the exploration bonus lives on the GPU: the HIP path has no CPU fallback")

    def _arg(self, t, name, shape, dtype):
        if not torch.is_tensor(t):
            raise ValueError(f"step(): {name} must be a tensor on the bonus's device")
        if tuple(t.shape) != shape:
            raise ValueError(f"step(): {name} of shape {shape} required, got {tuple(t.shape)}")
        if t.dtype != dtype:
            raise ValueError(f"step(): {name} must be {dtype}, got {t.dtype}")
        if t.device != _lib.device_index(self.device):
            raise ValueError(f"step(): {name} is on {t.device}, the bonus on {self.device}")
        return t.contiguous()

    def _next_out(self):
        """the output set (codes, counts, bonus, reward + bonus) the next launch writes"""
        if self._out is None:
            dev, N = self.device, self.N
            self._out = [(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                          torch.empty(N, dtype=torch.float32, device=dev),
                          torch.empty(N, dtype=torch.float32, device=dev)) for _ in range(2)] + [0]
        out = self._out[self._out[2]]
        self._out[2] ^= 1
        return out

    def step(self, frame, reward=None, update=True):
        """frame: uint8 [N, 3, 84, 84], reward: None or float32 [N], both tensors on this object's device (a view that
        is not contiguous is copied first); ValueError otherwise, and nothing is launched.  Two launches; returns reward +
        bonus when a reward is given, else the bonus: float32 [N] from one of the two output sets used in turn.
        update=False looks the counts up without counting.  DrqError on a CPU device, after the checks."""
        frame = self._arg(frame, "frame", (self.N,) + self.FRAME_SHAPE, torch.uint8)
        if reward is not None:
            reward = self._arg(reward, "reward", (self.N,), torch.float32)
        self._on_gpu()
        codes, counts, bonus, total = self._next_out()
        with torch.cuda.device(self.device):
            launch("drq_explore_simhash_step", ptr(frame), self.N, self.bits, self.seed, self.beta, int(bool(update)),
                   ptr(self.table), ptr(codes), ptr(counts), ptr(bonus), ptr(reward),
                   None if reward is None else ptr(total), device=self.device)
            for t in (frame, reward):      # a caller's tensor may be freed right after step(): the launches still read it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
        self.codes, self.counts, self.last_bonus = codes, counts, bonus
        return bonus if reward is None else total

    def distinct(self):
        """the number of codes counted so far: a 0-d int64 tensor on the device, enqueued like everything else"""
        return torch.count_nonzero(self.table)

    def reset(self):
        """the table back to zero, enqueued on the current stream"""
        self.table.zero_()
        self.codes = self.counts = self.last_bonus = None

    # ---- checkpoints ---------------------------------------------------------------------
    def _config(self):
        return {"N": self.N, "bits": self.bits, "beta": self.beta, "seed": self.seed}

    def state_dict(self):
        """The bonus as a plain dict of CPU tensors and Python scalars: "format": 1, "kind", the configuration (N, bits,
        beta, seed) and the table in sparse form -- "index": int64 [K], the codes with a count that is not zero, in
        ascending order, and "count": int32 [K], their counts; a table of 2^24 entries is not written out in full.
        This SYNCHRONISES the object's device: the copies wait for every launch enqueued so far."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        index = torch.nonzero(self.table).reshape(-1)
        return {"format": 1, "kind": type(self).__name__, "config": self._config(), "index": host(index),
                "count": host(self.table[index])}

    def load_state_dict(self, sd):
        """Restores what state_dict() saved, into a fresh or a used object: the table is the saved one exactly, and the
        bonuses that follow are those of the object that was saved.  ValueError, with nothing changed, for a wrong
        "format" / "kind", a configuration that differs from this object's (every differing field is named) or an
        "index" / "count" pair that is no sparse table of 2^bits entries."""
        check_state(self, sd, self._config())
        index, count = sd.get("index"), sd.get("count")
        if not (torch.is_tensor(index) and torch.is_tensor(count) and index.dtype == torch.int64
                and count.dtype == torch.int32 and index.dim() == 1 and index.shape == count.shape):
            raise ValueError("SimHashBonus.load_state_dict(): index int64 [K] and count int32 [K] required")
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= self.table.numel()
                              or int(torch.unique(index).numel()) != index.numel()):
            raise ValueError(f"SimHashBonus.load_state_dict(): every index must be a code of {self.bits} bits, each once")
        self.table.zero_()
        self.table[index.to(self.device)] = count.to(self.device)
        self.codes = self.counts = self.last_bonus = None
