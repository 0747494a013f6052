"""Evaluation for the vectorised loop (new; the reference evaluates its one environment on the host, train.py:98-122,
stacks its frames in a FrameStackWrapper, dmc.py:87-109, and records the episodes with video.py).  The contract of the two
launches is in include/drqv2_hip.h, "evaluation".

  VecFrameStack   the 9-channel observation of N environments without a replay ring: push() is ONE launch
                  (drq_vec_stack_push), the FrameStackWrapper rule for all N at once
  VecVideo        a clip of mosaic images on the device: record() is ONE launch (drq_vec_video_record) that scales,
                  transposes and tiles the newest frames; save() writes .npy or an animated PNG with zlib and struct alone
  evaluate()      the protocol of INTEGRATION.md, "Episode statistics": the first k episodes of every environment, one wait
                  per `poll_every` steps

evaluate() draws from no generator (act_batch(..., eval_mode=True) does not) and touches no store, iterator or optimiser
state, so it may sit between any two training steps and leaves the training run bit for bit what it was.
"""
import os
import struct
import zlib
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import launch, ptr
from .replay import VecDeviceReplay, VecEpisodeStats, _on_gpu

FRAME_SHAPE = (3, 84, 84)
FRAME_BYTES = 3 * 84 * 84


def _pinned_stage(stage, k, t, device):
    """a host tensor -> the device through a pinned buffer of its shape and type, kept in stage[k]: a blocking copy"""
    held = stage.get(k)
    if held is None or held[0].shape != t.shape:
        held = stage[k] = (torch.empty(t.shape, dtype=t.dtype).pin_memory(), torch.empty(t.shape, dtype=t.dtype, device=device))
    held[0].copy_(t)
    held[1].copy_(held[0], non_blocking=False)
    return held[1]


class VecFrameStack:
    """The reference's FrameStackWrapper (dmc.py:87-109) for N environments on the device, without a replay ring:

        stack = VecFrameStack(num_envs=N, device="cuda")
        obs = stack.push(env.reset())                       # uint8 [N, 9, 84, 84]: every frame three times
        frame, reward, discount, first = env.step(agent.act_batch(obs, step, True))
        obs = stack.push(frame, first)                      # ONE launch (drq_vec_stack_push), nothing waits

    push(frame, first): an environment with first[e] holds its new frame three times, every other one drops its oldest
    frame and appends the new one.  The first push() after construction or reset() is a reset row for every environment
    whatever `first` says, like row 0 of the ring and call 0 of VecEpisodeStats.  TWO buffers are used in turn -- the
    launch reads one and writes the other, so they cannot overlap -- and a returned tensor is overwritten by the second
    push() after it, the convention of VecFrameReplay.observation(); a caller that keeps one longer clones it.
    observation() returns the newest stack again without a launch."""

    _row = VecDeviceReplay._row      # add()'s checks and messages

    def __init__(self, num_envs, device):
        self.N = int(num_envs)
        if self.N < 1:
            raise ValueError("num_envs must be >= 1")
        self.device = torch.device(device)
        self.obs_shape = (9, 84, 84)
        self._bufs = None           # the two stacks
        self._newest = None         # index of the buffer the last push() wrote; None: the next push() resets every environment
        self._at = 0                # index of the buffer the next push() writes
        self._stage = {}

    def reset(self):
        """The next push() is a reset row for every environment.  No launch."""
        self._newest = None

    def push(self, frame, first=None):
        """frame uint8 [N, 3, 84, 84], first bool / uint8 [N] or None = no environment was reset: the tensors of
        VecFrameReplay.add(), checked by the same rules (ValueError).  Tensors on the device go to the launch as they are
        and nothing waits; numpy arrays and host tensors are staged with a blocking copy.  Returns the stacks, uint8
        [N, 9, 84, 84] on the device."""
        N = self.N
        args = [self._row(frame, "frame", [(N,) + FRAME_SHAPE, (N, FRAME_BYTES)], (torch.uint8,)),
                None if first is None else self._row(first, "first", [(N,)], (torch.uint8, torch.bool))]
        _on_gpu(self, "the frame stacks live")
        if self._bufs is None:
            self._bufs = [ops._alloc((N,) + self.obs_shape, torch.uint8, self.device) for _ in range(2)]
        reset_all = self._newest is None
        prev, out = (None if reset_all else self._bufs[self._newest]), self._bufs[self._at]
        with torch.cuda.device(self.device):
            src = [t if t is None or t.is_cuda else _pinned_stage(self._stage, k, t, self.device) for k, t in enumerate(args)]
            launch("drq_vec_stack_push", ptr(prev), ptr(out), ptr(src[0]), ptr(src[1]), N, int(reset_all),
                   device=self.device)
            for t in src:           # a caller's tensor may be freed right after push(): the launch still reads it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
        self._newest, self._at = self._at, self._at ^ 1
        return out

    def observation(self):
        """The stacks the last push() returned; no launch.  DrqError before the first push()."""
        if self._newest is None:
            raise _lib.DrqError("observation(): no frame has been pushed yet")
        return self._bufs[self._newest]


# ---- animated PNG ------------------------------------------------------------------------------------------------
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _int_fps(fps):
    if isinstance(fps, bool) or int(fps) != fps or not 1 <= int(fps) <= 65535:
        raise ValueError(f"fps {fps!r}: an integer in 1 .. 65535 (the delay of a frame is 1 / fps seconds)")
    return int(fps)


def apng_bytes(frames, fps=20, level=6):
    """The animated PNG of uint8 [n, H, W, 3] images as bytes: 8-bit RGB, filter type 0 on every row; IHDR, acTL (n frames,
    num_plays 0 = for ever), then per frame an fcTL (the whole image, delay 1 / fps, dispose 0, blend 0) and its data --
    IDAT for frame 0, so that a plain PNG reader shows it, fdAT for the others -- with the sequence numbers 0, 1, 2, ...
    over the fcTL and fdAT chunks in file order, and IEND.  Standard library only."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise ValueError(f"frames: a non-empty uint8 [n, H, W, 3] array required, got {frames.dtype} {frames.shape}")
    fps = _int_fps(fps)
    n, H, W, _ = frames.shape
    out = [_PNG_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)),
           _chunk(b"acTL", struct.pack(">II", n, 0))]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)                  # column 0: the filter type of every row, 0
    seq = 0
    for i in range(n):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, 1, fps, 0, 0)))
        seq += 1
        rows[:, 1:] = frames[i].reshape(H, 3 * W)
        data = zlib.compress(rows.tobytes(), level)
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def _write_atomic(path, data):
    """path + ".tmp", flushed and fsynced, then renamed onto path, as checkpoint.save does"""
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(data)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def write_apng(path, frames, fps=20, level=6):
    """apng_bytes(frames, fps) into `path`, atomically.  Returns the number of bytes written."""
    data = apng_bytes(frames, fps, level)
    _write_atomic(os.fspath(path), data)
    return len(data)


def png_chunks(data):
    """[(type, payload)] of a PNG byte string; ValueError for a wrong signature, a chunk that runs past the end or a CRC
    that does not verify"""
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError("not a PNG file: wrong signature")
    chunks, at = [], 8
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError("truncated PNG chunk")
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        if at + 12 + n > len(data):
            raise ValueError(f"PNG chunk {kind!r} runs past the end of the file")
        payload = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if crc != zlib.crc32(kind + payload) & 0xFFFFFFFF:
            raise ValueError(f"PNG chunk {kind!r}: CRC mismatch")
        chunks.append((kind, payload))
        at += 12 + n
    return chunks


def _unfiltered(data, H, W):
    raw = np.frombuffer(zlib.decompress(data), np.uint8)
    if raw.size != H * (1 + 3 * W):
        raise ValueError("PNG image data of the wrong size")
    rows = raw.reshape(H, 1 + 3 * W)
    if rows[:, 0].any():
        raise ValueError("only filter type 0 is read")
    return rows[:, 1:].reshape(H, W, 3)


def read_apng(path):
    """(uint8 [n, H, W, 3], fps) of a file write_apng() / VecVideo.save() wrote.  ValueError for anything that is not of
    that form: another colour type or bit depth, interlacing, partial frames, a row filter, sequence numbers out of
    order, a frame whose delay differs from the first's."""
    with open(os.fspath(path), "rb") as f:
        chunks = png_chunks(f.read())
    kinds = [k for k, _ in chunks]
    if len(chunks) < 5 or kinds[0] != b"IHDR" or kinds[1] != b"acTL" or kinds[-1] != b"IEND":
        raise ValueError("not an animated PNG of this module: IHDR, acTL ... IEND expected")
    if len(chunks[0][1]) != 13 or len(chunks[1][1]) != 8:
        raise ValueError("IHDR / acTL of the wrong size")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    if (depth, colour, comp, filt, interlace) != (8, 2, 0, 0, 0) or W < 1 or H < 1:
        raise ValueError("only 8-bit RGB without interlacing is read")
    n, plays = struct.unpack(">II", chunks[1][1])
    body = chunks[2:-1]
    if n < 1 or len(body) != 2 * n:
        raise ValueError(f"acTL names {n} frames, the file holds {len(body)} chunks for them")
    frames, seq, delay = np.empty((n, H, W, 3), np.uint8), 0, None
    for i in range(n):
        (k0, ctl), (k1, data) = body[2 * i], body[2 * i + 1]
        if k0 != b"fcTL" or len(ctl) != 26 or k1 != (b"IDAT" if i == 0 else b"fdAT"):
            raise ValueError(f"frame {i}: fcTL and {'IDAT' if i == 0 else 'fdAT'} expected, got {k0!r}, {k1!r}")
        s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", ctl)
        if (s, w, h, x, y, dispose, blend) != (seq, W, H, 0, 0, 0, 0) or num < 1:
            raise ValueError(f"frame {i}: a full-frame fcTL with sequence number {seq}, dispose 0, blend 0 expected")
        seq += 1
        den = den or 100                                       # the format's meaning of a zero denominator
        if delay not in (None, (num, den)):
            raise ValueError(f"frame {i}: its delay differs from frame 0's")
        delay = (num, den)
        if i:
            if len(data) < 4 or struct.unpack(">I", data[:4])[0] != seq:
                raise ValueError(f"frame {i}: fdAT with sequence number {seq} expected")
            seq += 1
            data = data[4:]
        frames[i] = _unfiltered(data, H, W)
    num, den = delay
    return frames, (den // num if den % num == 0 else den / num)


class VecVideo:
    """A clip of the evaluation on the device (the reference's video.py keeps a list of host frames and hands it to
    imageio): image number i is a mosaic of the newest frames of the environments `envs`, GH x GW tiles of S x S pixels,
    S = 84 scale, channels last.

        video = VecVideo(num_envs=N, device="cuda")             # the first min(N, 16) environments, scale 2
        video.record(frame, stats.episodes_done, k)             # ONE launch (drq_vec_video_record), nothing waits
        video.save("eval_10000.png")                            # synchronises; an animated PNG (or .npy: the raw array)

    envs: the environments shown, distinct and in range (ValueError); default the first min(N, 16).  grid = (GH, GW):
    default GW = ceil(sqrt(M)), GH = ceil(M / GW); ValueError when it holds fewer than M tiles; tiles past M are black.
    scale 1 .. 4.  The clip is ONE uint8 tensor [max_frames, GH S, GW S, 3], allocated here.  record(frame, done, limit)
    writes image len(video) and counts it; with done (int32 [N], VecEpisodeStats.episodes_done) and limit > 0 the tile of
    an environment with done[e] >= limit -- one whose counted episodes are over -- is dimmed to a quarter.  Once max_frames
    are held, record() launches nothing and counts in `dropped`.  clear() starts over; clip() is the recorded part, a
    device view."""

    _row = VecDeviceReplay._row      # add()'s checks and messages

    def __init__(self, num_envs, device, envs=None, grid=None, scale=2, max_frames=512):
        self.N, self.scale, self.max_frames = int(num_envs), int(scale), int(max_frames)
        if self.N < 1 or self.max_frames < 1:
            raise ValueError("num_envs and max_frames must be >= 1")
        if not 1 <= self.scale <= 4 or self.scale != scale:
            raise ValueError(f"scale {scale!r}: an integer in 1 .. 4 required")
        envs = list(range(min(self.N, 16))) if envs is None else [int(e) for e in envs]
        if not envs or len(set(envs)) != len(envs) or min(envs) < 0 or max(envs) >= self.N:
            raise ValueError(f"envs {envs}: distinct environments in [0, {self.N}) required, at least one")
        M = len(envs)
        if grid is None:
            GW = int(np.ceil(np.sqrt(M)))
            while GW * GW < M:                                 # sqrt of a large square rounded down
                GW += 1
            grid = ((M + GW - 1) // GW, GW)
        GH, GW = (int(g) for g in grid)
        if GH < 1 or GW < 1 or GH * GW < M:
            raise ValueError(f"grid {GH} x {GW} holds fewer than the {M} environments shown")
        self.envs, self.grid = tuple(envs), (GH, GW)
        self.device = torch.device(device)
        S = 84 * self.scale
        self.image_shape = (GH * S, GW * S, 3)
        self.buffer = ops._alloc((self.max_frames,) + self.image_shape, torch.uint8, self.device)
        self._envs = torch.tensor(envs, dtype=torch.int32, device=self.device)      # checked above, once
        self._n = 0
        self.dropped = 0
        self._stage = {}

    def __len__(self):
        return self._n

    def clear(self):
        """Starts over: the next record() writes image 0.  No launch."""
        self._n = self.dropped = 0

    def clip(self):
        """uint8 [len(video), GH S, GW S, 3]: the recorded part of the clip, a view of the device tensor"""
        return self.buffer[:self._n]

    def record(self, frame, done=None, limit=0):
        """frame uint8 [N, 3, 84, 84] under add()'s rules; done int32 [N] on the device or None; limit >= 0."""
        N = self.N
        args = [self._row(frame, "frame", [(N,) + FRAME_SHAPE, (N, FRAME_BYTES)], (torch.uint8,)),
                None if done is None else self._row(done, "done", [(N,)], (torch.int32,))]
        limit = int(limit)
        if limit < 0:
            raise ValueError(f"record(): limit {limit} must be >= 0")
        _on_gpu(self, "the video clip lives")
        if self._n >= self.max_frames:
            self.dropped += 1
            return
        with torch.cuda.device(self.device):
            src = [t if t is None or t.is_cuda else _pinned_stage(self._stage, k, t, self.device) for k, t in enumerate(args)]
            launch("drq_vec_video_record", ptr(src[0]), ptr(self._envs), len(self.envs), ptr(src[1]), limit,
                   ptr(self.buffer[self._n]), self.grid[0], self.grid[1], self.scale, N, device=self.device)
            for t in src:           # a caller's tensor may be freed right after record(): the launch still reads it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
        self._n += 1

    def save(self, path, fps=20):
        """Writes the recorded clip to `path`: ".npy" the raw uint8 [n, GH S, GW S, 3] array, ".png" an animated PNG
        (apng_bytes: zlib and struct alone; a plain PNG reader shows image 0).  SYNCHRONISES (the copy to the host waits for
        every record() enqueued so far) and compresses on the host.  Atomic, like checkpoint.save.  DrqError for an empty
        clip, ValueError for another extension.  Returns the number of bytes written."""
        path = os.fspath(path)
        ext = os.path.splitext(path)[1].lower()
        if ext not in (".npy", ".png"):
            raise ValueError(f"save(): {path!r}: .npy or .png required")
        fps = _int_fps(fps)
        if self._n == 0:
            raise _lib.DrqError("save(): the clip is empty")
        host = self.clip().cpu().numpy()
        if ext == ".png":
            return write_apng(path, host, fps)
        import io
        buf = io.BytesIO()
        np.save(buf, host)
        _write_atomic(path, buf.getvalue())
        return buf.tell()


# ---- the runner --------------------------------------------------------------------------------------------------
EvalResult = namedtuple("EvalResult", "snapshot steps frames")
EvalResult.__doc__ = """What evaluate() returns: snapshot, the EpisodeSnapshot of the completed statistics (mean_return,
records, ...); steps, the env.step() calls made; frames, the images this call recorded into `video` (0 without one)."""


def evaluate(agent, env, episodes_per_env=1, step=0, *, stats=None, stack=None, video=None, poll_every=50, max_steps=None):
    """Runs the first `episodes_per_env` episodes of EVERY environment of `env` under agent.act_batch(obs, step, True) and
    returns EvalResult(snapshot, steps, frames) -- train.py:98-122 for N lockstep environments ("until K episodes have
    finished" would favour short ones).  `env` needs reset() -> frame and step(action) -> (frame, reward, discount, first)
    with VecReach's signatures.

        frame = env.reset(); obs = stack.push(frame) after stack.reset(); stats.step(zeros)
        every iteration:  action = agent.act_batch(obs, step, True);  frame, reward, discount, first = env.step(action)
                          obs = stack.push(frame, first);  stats.step(reward, first)
        video, if given:  video.record(frame, stats.episodes_done, episodes_per_env) behind the stats.step() of the same
                          row, the reset row included

    That order is part of the contract: stats.step() raises episodes_done[e] on the row that carries first, so the last
    frame of a counted episode is recorded as it is and the first frame of the next one dimmed.  Every `poll_every`
    iterations stats.read() -- the one wait -- and the loop ends when the snapshot is complete; the iterations between
    completion and that read are run and recorded (dimmed) but count nowhere.  stats (its max_episodes_per_env must
    equal episodes_per_env: ValueError; it is reset()) and stack are built when not given.  max_steps defaults to
    episodes_per_env * (env.episode_length + 1) + poll_every where the environment has an episode_length and is required
    otherwise (ValueError); reaching it without completion raises DrqError.
    Nothing here draws from a generator or touches a store, an iterator or optimiser state; like act_batch() it first
    completes a deferred optimiser step (inside the first act_batch())."""
    k, poll_every = int(episodes_per_env), int(poll_every)
    if k < 1 or poll_every < 1:
        raise ValueError("episodes_per_env and poll_every must be >= 1")
    if stats is not None and stats.limit != k:
        raise ValueError(f"evaluate(): stats counts max_episodes_per_env = {stats.limit}, episodes_per_env is {k}")
    if max_steps is None:
        length = getattr(env, "episode_length", None)
        if length is None:
            raise ValueError("evaluate(): max_steps is required for an environment without an episode_length")
        max_steps = k * (int(length) + 1) + poll_every
    max_steps = int(max_steps)
    frame = env.reset()
    N, device = int(frame.shape[0]), frame.device
    if stats is None:
        stats = VecEpisodeStats(N, device, log_size=max(1024, k * N), max_episodes_per_env=k)
    else:
        stats.reset()
    if stack is None:
        stack = VecFrameStack(N, device)
    stack.reset()
    held = len(video) if video is not None else 0
    obs = stack.push(frame)
    stats.step(torch.zeros(N, dtype=torch.float32, device=device))
    if video is not None:
        video.record(frame, stats.episodes_done, k)
    steps = 0
    while True:
        for _ in range(min(poll_every, max_steps - steps)):
            action = agent.act_batch(obs, step, True)
            frame, reward, discount, first = env.step(action)
            obs = stack.push(frame, first)
            stats.step(reward, first)
            if video is not None:
                video.record(frame, stats.episodes_done, k)
            steps += 1
        snap = stats.read()
        if snap.complete:
            return EvalResult(snap, steps, (len(video) - held) if video is not None else 0)
        if steps >= max_steps:
            raise _lib.DrqError(f"evaluate(): {snap.episodes} of {k * N} episodes after max_steps = {max_steps} steps")
