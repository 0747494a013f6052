"""Count-based exploration bonus for vectorised collection (new; the reference explores by the noise of its policy alone,
drqv2.py:164-175, and every reward its replay sees is the environment's own).

SimHashBonus is the bonus of "#Exploration" (Tang et al. 2017) on the frames of N lockstep environments where they
already are: a SimHash of every frame (a 21 x 21 grid of block sums, centred, `bits` random +-1 projections, their signs),
a table of 2^bits visit counts in HBM, bonus = beta / sqrt(count).  One call is two launches on the current stream
(csrc/explore.hip, drq_explore_simhash_step) and no host wait; the contract is spelled out to the bit in
include/drqv2_hip.h ("exploration bonus") and restated in numpy by tests/simhash_oracle.py.

KnnBonus is the state-entropy bonus of RE3 (Seo et al., ICML 2021) beside it: beta * log(1 + the distance to the k-th nearest
neighbour in the feature space of a fixed random encoder), looked up among the rows the ring holds at the moment a batch
is drawn and added to the batch's reward in place -- update() is untouched, an IndexedBatch carries its reward tensor.
RandomFeatures is that encoder.  One call is two launches (csrc/knn.hip, drq_explore_knn: the k-th nearest of B rows among
all stored rows without the B x M matrix of distances) and no host wait; the contract is in include/drqv2_hip.h ("k-NN
bonus") and restated in numpy by tests/knn_oracle.py.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import launch, ptr
from .checkpoint import check_state, host


MAX_BITS = 24        # DRQ_SIMHASH_MAX_BITS
KNN_MAX_DIM, KNN_MAX_K, KNN_CHUNK = 64, 8, 128       # DRQ_KNN_MAX_DIM, DRQ_KNN_MAX_K, DRQ_KNN_CHUNK


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


def _int_in(value, lo, hi, name):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an int in {lo} .. {hi}, got {value!r}")
    return value


class RandomFeatures:
    """
        features = RandomFeatures(obs_shape=(9, 84, 84), dim=50, device="cuda", seed=0)
        y = features(store.observation())        # uint8 [N, 9, 84, 84] -> float32 [N, dim]

    RE3's random encoder: a frozen drqv2.Encoder, Linear(39200, dim) and LayerNorm(dim), initialised as the agent's own
    modules are (utils.weight_init) but under a forked torch generator seeded with `seed`, so neither construction nor a
    call moves the global CPU or GPU generators, and two objects of one seed hold the same weights.  It is never trained.
    A call runs under no_grad: the four convolutions on the HIP encoder forward, the projection and the norm in plain
    torch (N rows: plumbing), in float64 and rounded to float32 once.  ValueError for a wrong shape, dtype or device before anything is launched; DrqError on a
    CPU device after the checks.  state_dict() holds the configuration and the seed only: the weights follow from them."""

    def __init__(self, obs_shape=(9, 84, 84), dim=50, device="cuda", seed=0):
        shape = tuple(int(s) for s in obs_shape)
        if len(shape) != 3 or shape[1:] != (84, 84) or shape[0] not in (3, 6, 9, 12):
            raise ValueError(f"obs_shape must be (C, 84, 84) with C in 3, 6, 9, 12, got {obs_shape!r}")
        self.obs_shape, self.dim = shape, _int_in(dim, 1, KNN_MAX_DIM, "dim")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        self.seed = seed & 0xFFFFFFFF
        self.device = torch.device(device)
        import drqv2        # here: drqv2 imports this package
        with torch.random.fork_rng(devices=[]):      # built on the CPU: only the CPU generator is drawn from
            torch.default_generator.manual_seed(self.seed)      # the CPU generator alone: torch.manual_seed seeds the GPUs too
            self.encoder = drqv2.Encoder(shape)
            self.head = torch.nn.Sequential(torch.nn.Linear(self.encoder.repr_dim, self.dim), torch.nn.LayerNorm(self.dim))
            self.head.apply(drqv2.utils.weight_init)
        # the projection sums 39,200 terms: in float64, so that the features do not move with the accumulation order of
        # whatever GEMM serves nn.Linear; they are rounded to float32 once, at the end
        self.head.double()
        for m in (self.encoder, self.head):
            m.to(self.device).requires_grad_(False).eval()

    def __call__(self, obs):
        if not torch.is_tensor(obs):
            raise ValueError("obs must be a tensor on the encoder's device")
        if obs.dim() != 4 or tuple(obs.shape[1:]) != self.obs_shape or obs.shape[0] < 1:
            raise ValueError(f"obs of shape [N, {', '.join(map(str, self.obs_shape))}] required, got {tuple(obs.shape)}")
        if obs.dtype != torch.uint8:
            raise ValueError(f"obs must be uint8, got {obs.dtype}")
        if obs.device != _lib.device_index(self.device):
            raise ValueError(f"obs is on {obs.device}, the encoder on {self.device}")
        if self.device.type != "cuda":
            raise _lib.DrqError("the random encoder runs on the GPU: the HIP path has no CPU fallback")
        with torch.no_grad(), torch.cuda.device(self.device):
            return self.head(self.encoder(obs.contiguous()).double()).float().contiguous()

    def _config(self):
        return {"obs_shape": self.obs_shape, "dim": self.dim, "seed": self.seed}

    def state_dict(self):
        return {"format": 1, "kind": type(self).__name__, "config": self._config()}

    def load_state_dict(self, sd):
        """nothing to restore: ValueError unless `sd` is the state of an object of this configuration and seed"""
        check_state(self, sd, self._config())


class KnnBatches:
    """What KnnBonus.batches(it) returns: the batches of `it` with the bonus applied when they are HANDED OUT.  prefetch()
    is the inner iterator's own, so its look-ahead batch stays as the store drew it and a checkpoint of the inner
    iterator resumes bit for bit."""

    def __init__(self, bonus, it):
        self.bonus, self.it = bonus, it

    def __iter__(self):
        return self

    def __next__(self):
        return self.bonus.apply(next(self.it))

    def prefetch(self):
        self.it.prefetch()


class KnnBonus:
    """
        bonus = KnnBonus(store, dim=50, k=3, beta=0.05, candidates=None, seed=0)     # store: VecDeviceReplay / VecFrameReplay
        store.add(...); bonus.observe(y)         # y float32 [N, dim] on the device: the features of the row just added
        it = bonus.batches(iter(store))          # batches with reward += beta * log1p(dist), in place
        agent.update(it, step)

    A feature table float32 [R N, dim] lives beside the ring: observe(y) copies y into the slots of the row the store
    added last, rows ((T - 1) mod R) N .. + N, a torch slice copy on the current stream.  Every row needs its features:
    observe() twice for one row, or after more than one add(), raises ValueError (a skipped row would silently pair
    features with the wrong frames), and the bonus is made before the store's first add().

    apply(batch) is one drq_explore_knn call on the batch's position slots (`batch.slots`, the store's last_index[2]):
    dist = the distance from the slot's features to its k-th nearest neighbour among the live rows, min(T, R) N of them,
    the slot itself excluded by index; then batch[2].add_(beta * log1p(dist)).  A slot outside the live rows gets 0: the
    rows of a demonstration partition sit at R N and above and so carry no bonus.  With fewer than k other candidates
    the bonus is 0 as well.  last_dist and last_bonus are the float32 [B] tensors of the newest call.  Nothing waits.
    candidates=M bounds the work on a large ring: stride = ceil(live / M) and an offset drawn per call from a
    numpy RandomState(seed) of this object's own pick every stride-th row; None looks at all of them.
    beta is a plain attribute.  state_dict() / load_state_dict() go through checkpoint.save(..., bonus=...)."""

    def __init__(self, store, dim=50, k=3, beta=0.05, candidates=None, seed=0):
        if not all(isinstance(getattr(store, a, None), int) for a in ("R", "N", "T")) or not hasattr(store, "device"):
            raise ValueError("store must be a VecDeviceReplay or VecFrameReplay")
        self.dim, self.k = _int_in(dim, 1, KNN_MAX_DIM, "dim"), _int_in(k, 1, KNN_MAX_K, "k")
        self.beta = float(beta)
        if not math.isfinite(self.beta) or self.beta < 0:
            raise ValueError(f"beta must be a finite number >= 0, got {beta!r}")
        self.candidates = None if candidates is None else _int_in(candidates, 1, 2 ** 62, "candidates")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        if store.T != 0:
            raise ValueError(f"the store already holds {store.T} rows without features: make the bonus before the first add() "
                             "(a resumed run loads both from the checkpoint)")
        self.store, self.seed = store, seed & 0xFFFFFFFF
        self.R, self.N, self.device = store.R, store.N, torch.device(store.device)
        self.table = torch.zeros((self.R * self.N, self.dim), dtype=torch.float32, device=self.device)
        self.rows = 0               # rows observed: the store's T at the last observe()
        self.rng = np.random.RandomState(self.seed)
        self.last_dist = self.last_bonus = None
        self.last_stride, self.last_offset = 1, 0
        self._ws = None

    def _on_gpu(self):
        if self.device.type != "cuda":
            raise _lib.DrqError("the k-NN bonus lives on the GPU: the HIP path has no CPU fallback")

    @property
    def live(self):
        """the rows of the table that hold features: min(T, R) N"""
        return min(self.rows, self.R) * self.N

    def observe(self, y):
        """y: float32 [N, dim] on the store's device, the features of the row the store added last."""
        if not torch.is_tensor(y):
            raise ValueError("observe(): y must be a tensor on the store's device")
        if tuple(y.shape) != (self.N, self.dim):
            raise ValueError(f"observe(): y of shape {(self.N, self.dim)} required, got {tuple(y.shape)}")
        if y.dtype != torch.float32:
            raise ValueError(f"observe(): y must be float32, got {y.dtype}")
        if y.device != _lib.device_index(self.device):
            raise ValueError(f"observe(): y is on {y.device}, the store on {self.device}")
        T = self.store.T
        if T == self.rows:
            raise ValueError(f"observe(): row {T - 1} has its features already (observe() once after every add())")
        if T != self.rows + 1:
            raise ValueError(f"observe(): the store has added {T - self.rows} rows since the last observe(): the features of "
                             f"rows {self.rows} .. {T - 2} are missing")
        self._on_gpu()
        lo = ((T - 1) % self.R) * self.N
        self.table[lo:lo + self.N].copy_(y)
        self.rows = T

    def lattice(self):
        """(stride, offset) of the next call; with `candidates` the offset is one randint draw of the object's RandomState"""
        if self.candidates is None:
            return 1, 0
        stride = max(1, -(-self.live // self.candidates))
        return stride, int(self.rng.randint(0, stride))

    def apply(self, batch):
        """Adds the bonus to batch[2] in place and returns the batch (its class, weights and update_priorities are what
        they were).  ValueError, nothing drawn or launched: a batch without position slots (a materialised one: the store
        needs indexed=True), a reward that is no float32 [B, 1] on this device."""
        slots, reward = getattr(batch, "slots", None), batch[2] if isinstance(batch, tuple) and len(batch) == 5 else None
        if not torch.is_tensor(slots) or slots.dtype != torch.int64 or slots.dim() != 1 or slots.numel() < 1:
            raise ValueError("apply(): an indexed batch of a VecDeviceReplay / VecFrameReplay required (batch.slots int64 [B])")
        B = slots.numel()
        if not torch.is_tensor(reward) or reward.dtype != torch.float32 or tuple(reward.shape) != (B, 1):
            raise ValueError(f"apply(): the batch's reward must be float32 [{B}, 1]")
        dev = _lib.device_index(self.device)
        if slots.device != dev or reward.device != dev:
            raise ValueError(f"apply(): the batch is on {slots.device}, the bonus on {self.device}")
        self._on_gpu()
        live = self.live
        stride, offset = self.lattice()
        slots = slots.contiguous()
        dist = torch.empty(B, dtype=torch.float32, device=self.device)
        need = _lib.load().drq_explore_knn_ws_bytes(B, live, stride)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty(max(1, need // 4), dtype=torch.float32, device=self.device)
        launch("drq_explore_knn", ptr(self.table), self.table.shape[0], self.dim, live, ptr(slots), B, self.k, stride, offset,
               ptr(dist), ptr(self._ws), self._ws.numel() * 4, device=self.device)
        with torch.cuda.device(self.device):
            slots.record_stream(torch.cuda.current_stream())
            self.last_dist, self.last_bonus = dist, self.beta * torch.log1p(dist)
            reward.add_(self.last_bonus.view(B, 1))
        self.last_stride, self.last_offset = stride, offset
        return batch

    def batches(self, it):
        """an iterator with __next__ and prefetch() over the batches of `it` (iter(store)), the bonus applied at hand-out"""
        return KnnBatches(self, it)

    # ---- checkpoints ---------------------------------------------------------------------
    def _config(self):
        return {"R": self.R, "N": self.N, "dim": self.dim, "k": self.k, "beta": self.beta, "candidates": self.candidates,
                "seed": self.seed}

    def state_dict(self):
        """The bonus as a plain dict of CPU tensors and Python scalars: "format": 1, "kind", the configuration (R, N, dim, k,
        beta, candidates, seed), "rows" (the row counter), "table" (the live prefix, float32 [min(rows, R) N, dim]) and
        "rng" (the RandomState as the stores save theirs).  This SYNCHRONISES the object's device."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        name, key, pos, has_gauss, cached = self.rng.get_state()
        return {"format": 1, "kind": type(self).__name__, "config": self._config(), "rows": self.rows,
                "table": host(self.table[:self.live]),
                "rng": (name, torch.from_numpy(key.astype(np.int64)), int(pos), int(has_gauss), float(cached))}

    def load_state_dict(self, sd):
        """Restores what state_dict() saved, into a fresh or a used object; ValueError, with nothing changed, for a wrong
        "format" / "kind", a configuration that differs (every differing field is named), a row counter or a table that
        does not fit, a missing RandomState.  The rows above the live ones are zero afterwards."""
        check_state(self, sd, self._config())
        rows = sd.get("rows")
        if isinstance(rows, bool) or not isinstance(rows, int) or rows < 0:
            raise ValueError(f"KnnBonus.load_state_dict(): rows {rows!r} is no row counter")
        live = min(rows, self.R) * self.N
        check_state(self, sd, tensors={"table": ((live, self.dim), torch.float32)})
        rng = sd.get("rng")
        if (not isinstance(rng, (tuple, list)) or len(rng) != 5 or not torch.is_tensor(rng[1]) or rng[1].numel() != 624
                or not 0 <= int(rng[2]) <= 624):
            raise ValueError("KnnBonus.load_state_dict(): no RandomState in the saved state")
        self.table[:live].copy_(sd["table"])
        self.table[live:].zero_()
        self.rows = rows
        self.rng.set_state((rng[0], rng[1].numpy().astype(np.uint32), int(rng[2]), int(rng[3]), float(rng[4])))
        self.last_dist = self.last_bonus = None
