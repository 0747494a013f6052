"""Visual distractions for vectorised collection (new; the reference trains and evaluates on the clean frames of
dm_control, dmc.py).

The Distracting Control Suite (Stone et al. 2021) and DMControl-GB (Hansen & Wang 2021) ask whether a pixel agent still
works when the image changes in ways that do not matter, and perturb exactly three things: the background, the colours
and the camera -- during training, or only at evaluation to measure the generalisation gap.  FrameDistractor applies the
three to the frames of N lockstep environments where they already are: one launch per step on the current stream
(csrc/vecdistract.hip, drq_vec_distract) and no host wait.  VecDistract wraps a device environment so that everything
that takes one -- the rings, evaluate(), VecVideo, checkpoint.save / load -- takes the distracted one unchanged.  The
contract is spelled out to the bit in include/drqv2_hip.h ("distractions") and restated in numpy by
tests/vec_distract_oracle.py.
"""
import torch

from . import _lib
from ._lib import launch, ptr
from .checkpoint import check_state, host


MAX_CAMERA, MAX_COLOR, MAX_BANK = 8, 128, 65536      # DRQ_DISTRACT_MAX_CAMERA, _COLOR, _BANK
FRAME_SHAPE = (3, 84, 84)

# the presets of difficulty(): (camera, color, background_alpha), the background being noise.  "hard" is every strength at
# the end of its range but the colour, whose end (gains 0.5 .. 1.5, offsets of +-64) leaves the built-in tasks' 64 / 255
# discs no longer told apart by eye either
PRESETS = {"easy": (2, 16, 64), "medium": (4, 48, 128), "hard": (8, 96, 256)}


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an int in {lo} .. {hi}, got {v!r}")
    return v


def parse_spec(spec):
    """The keyword arguments of FrameDistractor from the text of a command line: a preset name ("easy", "medium", "hard")
    or a comma-separated list of camera=P, camera_period=K, color=C, background=none|noise, alpha=A, dynamic=0|1, e.g.
    "camera=4,color=32,background=noise".  ValueError names what it does not understand."""
    spec = str(spec).strip()
    if spec in PRESETS:
        return FrameDistractor.difficulty(spec)
    names = {"camera": "camera", "camera_period": "camera_period", "color": "color", "alpha": "background_alpha",
             "dynamic": "dynamic", "background": "background"}
    out = {}
    for item in filter(None, (s.strip() for s in spec.split(","))):
        k, eq, v = (s.strip() for s in item.partition("="))
        if not eq or k not in names or names[k] in out:
            raise ValueError(f"distractions {spec!r}: {item!r} is not one of {', '.join(sorted(names))}=VALUE, each once, "
                             f"nor is the whole one of {', '.join(PRESETS)}")
        if k == "background":
            if v not in ("none", "noise"):
                raise ValueError(f"distractions {spec!r}: background=none or background=noise, got {v!r}")
            out["background"] = v
        else:
            try:
                out[names[k]] = int(v)
            except ValueError:
                raise ValueError(f"distractions {spec!r}: {k} takes an integer, got {v!r}") from None
            if k == "dynamic":
                if out["dynamic"] not in (0, 1):
                    raise ValueError(f"distractions {spec!r}: dynamic=0 or dynamic=1")
                out["dynamic"] = bool(out["dynamic"])
    if not out:
        raise ValueError(f"distractions {spec!r}: nothing to apply")
    return out


class FrameDistractor:
    """
        distractor = FrameDistractor(num_envs=N, device="cuda", seed=0, camera=4, camera_period=4, color=32,
                                     background="noise", background_alpha=256, key=env.background_key(), dynamic=True)
        frame = distractor.apply(env.reset())                  # uint8 [N, 3, 84, 84]; the first call resets every lane
        frame = distractor.apply(frame, first)                 # first: the flags env.step() returned

    Per environment and episode a hash of (seed, environment, episode count) draws a camera offset in [-camera, camera]
    pixels per axis (edge pixels are replicated) and, with dynamic, a sweep of 0 .. 2 pixels per camera_period steps; a
    gain in 1 +- color / 256 and an offset within +-color / 2 per channel for the foreground; and a background -- "noise"
    (smooth value noise that drifts by up to 2 pixels a step) or a clip of a bank the caller supplies, a uint8 tensor
    [M, F, 3, 84, 84] on the device (M clips of F frames, played forward and backward in turn) -- blended over the clean
    background with weight background_alpha / 256.  dynamic=False freezes all three for the length of an episode.

    Which pixels are background is decided by `key`, the clean background of the renderer, uint8 [3, 84, 84]: a pixel
    that equals the key in all three channels is background, every other one foreground.  key="env" takes it from the
    environment VecDistract wraps (env.background_key()); key=None runs un-keyed -- every pixel is foreground, camera and
    colour only -- and a background then is a ValueError.

    Every return is a device tensor written by a launch on the current stream; nothing waits for the GPU.  apply() writes
    into TWO output buffers used in turn, as the device environments and VecFrameReplay.observation() do: a returned
    tensor is overwritten by the second apply() / render() call after it, so a caller that keeps one longer clones it;
    and the frame given must not be the buffer the call writes (the library refuses frames that overlap).

    The first apply() and the first after reset() start a new episode in every environment whatever `first` says.
    render(frame) draws the distracted frame of the state as it is, without a state step: after apply(frame, ...) it
    returns that frame again, and it is what a restored distractor shows before its next step.  state_dict() /
    load_state_dict() carry the configuration and the two state words per environment; the bank and the key are
    configuration by shape only, and the caller supplies the tensors again."""

    def __init__(self, num_envs, device, seed=0, camera=0, camera_period=4, color=0, background="none",
                 background_alpha=256, key=None, dynamic=True):
        self.N = int(num_envs)
        if self.N < 1:
            raise ValueError("num_envs must be >= 1")
        self.camera = _int_in("camera", camera, 0, MAX_CAMERA)
        self.camera_period = _int_in("camera_period", camera_period, 1, 2 ** 31 - 1)
        self.color = _int_in("color", color, 0, MAX_COLOR)
        self.background_alpha = _int_in("background_alpha", background_alpha, 0, 256)
        if not isinstance(dynamic, (bool, int)) or dynamic not in (0, 1):
            raise ValueError(f"dynamic must be True or False, got {dynamic!r}")
        self.dynamic = bool(dynamic)
        self.seed = int(seed) & 0xFFFFFFFF
        self.device = dev = torch.device(device)
        self.bank = None
        if torch.is_tensor(background):
            b = background
            if b.dim() != 5 or tuple(b.shape[2:]) != FRAME_SHAPE or b.shape[0] < 1 or b.shape[1] < 1:
                raise ValueError(f"background: a bank is [M, F, 3, 84, 84] with M, F >= 1, got {tuple(b.shape)}")
            if b.shape[0] > MAX_BANK or b.shape[1] > MAX_BANK:
                raise ValueError(f"background: a bank holds at most {MAX_BANK} clips of {MAX_BANK} frames, got {tuple(b.shape[:2])}")
            if b.dtype != torch.uint8:
                raise ValueError(f"background: a bank must be {torch.uint8}, got {b.dtype}")
            if b.device != _lib.device_index(self.device):
                raise ValueError(f"background: the bank is on {b.device}, the distractor on {dev}")
            if not b.is_contiguous():
                raise ValueError("background: the bank must be contiguous (it is read in place, never copied)")
            self.bank, self.background = b, "bank"
        elif background in ("none", "noise"):
            self.background = background
        else:
            raise ValueError(f"background must be \"none\", \"noise\" or a uint8 bank tensor [M, F, 3, 84, 84], got {background!r}")
        self.key, self.key_from_env = None, False
        if isinstance(key, str):
            if key != "env":
                raise ValueError(f"key must be None, \"env\" or a uint8 tensor [3, 84, 84], got {key!r}")
            self.key_from_env = True
        elif key is not None:
            self.set_key(key)
        elif self.background != "none":
            raise ValueError(f"background {self.background!r} without a key: which pixels are background is decided by "
                             "comparing with the clean background image (key=), or by the environment's (key=\"env\")")
        self.episode = torch.zeros(self.N, dtype=torch.int32, device=dev)      # uint32 on the device
        self.t = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self._started = False       # False: the next apply() starts a new episode in every environment
        self._out = None            # two frame buffers, then the index of the next

    @classmethod
    def difficulty(cls, name):
        """The keyword arguments of three fixed strengths, "easy", "medium" and "hard": camera, color and
        background_alpha of PRESETS over a noise background (which needs a key: key="env" under VecDistract)."""
        if name not in PRESETS:
            raise ValueError(f"difficulty {name!r}: one of {', '.join(PRESETS)}")
        camera, color, alpha = PRESETS[name]
        return {"camera": camera, "color": color, "background": "noise", "background_alpha": alpha}

    def _on_gpu(self):
        if self.device.type != "cuda":
            raise _lib.DrqError("the distractions live on the GPU: the HIP path has no CPU fallback")

    def set_key(self, key):
        """The clean background the frames are compared with: uint8 [3, 84, 84] on this object's device (ValueError
        otherwise).  VecDistract calls it for key="env"."""
        if not torch.is_tensor(key) or tuple(key.shape) != FRAME_SHAPE or key.dtype != torch.uint8:
            raise ValueError("key must be None, \"env\" or a uint8 tensor [3, 84, 84]" +
                             (f", got {key.dtype} {tuple(key.shape)}" if torch.is_tensor(key) else f", got {key!r}"))
        if key.device != _lib.device_index(self.device):
            raise ValueError(f"key is on {key.device}, the distractor on {self.device}")
        self.key = key.contiguous().clone()

    def _arg(self, t, what, name, shape, dtypes):
        if not torch.is_tensor(t):
            raise ValueError(f"{what}(): {name} must be a tensor on the distractor's device")
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}(): {name} of shape {shape} required, got {tuple(t.shape)}")
        if t.dtype not in dtypes:
            raise ValueError(f"{what}(): {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if t.device != _lib.device_index(self.device):
            raise ValueError(f"{what}(): {name} is on {t.device}, the distractor on {self.device}")
        return t.contiguous()

    def _next_out(self):
        if self._out is None:
            self._out = [torch.empty((self.N,) + FRAME_SHAPE, dtype=torch.uint8, device=self.device) for _ in range(2)] + [0]
        out = self._out[self._out[2]]
        self._out[2] ^= 1
        return out

    def _launch(self, what, frame, first, reset_all, hold):
        frame = self._arg(frame, what, "frame", (self.N,) + FRAME_SHAPE, (torch.uint8,))
        if first is not None:
            first = self._arg(first, what, "first", (self.N,), (torch.uint8, torch.bool))
        if self.key_from_env and self.key is None:
            raise ValueError(f"{what}(): key=\"env\" takes the key from the environment VecDistract wraps; set_key() gives one by hand")
        self._on_gpu()
        out = self._next_out()
        M, F = (0, 0) if self.bank is None else self.bank.shape[:2]
        with torch.cuda.device(self.device):
            launch("drq_vec_distract", ptr(frame), ptr(first), ptr(self.key), ptr(self.bank), ptr(self.episode), ptr(self.t),
                   self.N, self.seed, int(reset_all), int(hold), self.camera, self.camera_period, self.color,
                   ("none", "noise", "bank").index(self.background), self.background_alpha, int(self.dynamic), int(M), int(F),
                   ptr(out), device=self.device)
            for t in (frame, first):        # a caller's tensor may be freed right after the call: the launch still reads it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
        return out

    def apply(self, frame, first=None):
        """frame: uint8 [N, 3, 84, 84]; first: None (no environment was reset) or uint8 / bool [N], the flags of the step
        that made the frame; both tensors on this object's device (a view that is not contiguous is copied first);
        ValueError otherwise, and nothing is launched.  One launch: an environment with first[e] starts a new episode
        (new draws, t = 0), every other one advances t; returns the distracted frames, uint8 [N, 3, 84, 84], from one of
        the two buffers used in turn.  DrqError on a CPU device, after the checks."""
        out = self._launch("apply", frame, first, not self._started, False)
        self._started = True
        return out

    def render(self, frame):
        """The distracted `frame` under the state as it is: the same launch without its state step (hold = 1 of the
        entry), into the next of the two buffers.  DrqError before the first apply() of a distractor that was not
        restored from a started one."""
        if not self._started:
            raise _lib.DrqError("render(): call apply() or load_state_dict() first")
        return self._launch("render", frame, None, False, True)

    def reset(self):
        """The next apply() starts a new episode in every environment.  No launch."""
        self._started = False

    def state(self):
        """Host copies of the state words, for tests: {"episode": uint32 [N], "t": uint32 [N]}.  This SYNCHRONISES."""
        import numpy as np
        return {k: getattr(self, k).cpu().numpy().view(np.uint32) for k in ("episode", "t")}

    # ---- checkpoints ---------------------------------------------------------------------
    def _config(self):
        M, F = (0, 0) if self.bank is None else (int(s) for s in self.bank.shape[:2])
        return {"N": self.N, "seed": self.seed, "camera": self.camera, "camera_period": self.camera_period,
                "color": self.color, "background": self.background, "bank_clips": M, "bank_frames": F,
                "background_alpha": self.background_alpha, "keyed": self.key is not None or self.key_from_env,
                "dynamic": self.dynamic}

    def state_dict(self):
        """The distractor as a plain dict of CPU tensors and Python scalars: "format": 1, "kind", the configuration (N,
        seed, the strengths, the background's kind, the bank's M and F, whether there is a key) and per environment
        episode and t (int32 tensors that hold the uint32 bits), and "started".  The bank and the key are not in it.
        This SYNCHRONISES the object's device: the copies wait for every launch enqueued so far."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return {"format": 1, "kind": type(self).__name__, "config": self._config(), "started": self._started,
                "episode": host(self.episode), "t": host(self.t)}

    def _check(self, sd):
        check_state(self, sd, self._config(), {"episode": self.episode, "t": self.t})

    def load_state_dict(self, sd):
        """Restores what state_dict() saved, into a fresh or a used object built with the same arguments (and given the
        same bank and key by the caller).  ValueError, with nothing changed, for a wrong "format" / "kind", a
        configuration that differs from this object's (every differing field is named) or state tensors of another
        shape."""
        self._check(sd)
        self.episode.copy_(sd["episode"])
        self.t.copy_(sd["t"])
        self._started = bool(sd.get("started", True))


class VecDistract:
    """A device environment behind a FrameDistractor: the same interface, distracted frames.

        env = VecDistract(VecReach(num_envs=N, device="cuda"), FrameDistractor(N, "cuda", key="env", **FrameDistractor.difficulty("medium")))
        frame = env.reset();  frame, reward, discount, first = env.step(action)

    `env` is anything with the interface of the built-in tasks (reset, step, render, state_dict, load_state_dict; N, A,
    device, episode_length, action_repeat, last_substeps).  reset() and step() return the distracted frame beside the
    environment's own reward, discount and first, two launches per call and no wait; render() draws the current
    distracted frame again without advancing anything; image() is the renderer-shaped image of the distracted frame
    (drq_vec_reach_image).  A returned frame is one of the distractor's two buffers: it is overwritten by the second
    reset() / step() / render() after it.  state_dict() nests the environment's and the distractor's, so the wrapper goes
    wherever an environment goes: checkpoint.save / load (env=), evaluate(), VecVideo."""

    IMAGE_SIZES = (84, 168, 252, 336)

    def __init__(self, env, distractor):
        if not isinstance(distractor, FrameDistractor):
            raise ValueError(f"distractor must be a FrameDistractor, got {type(distractor).__name__}")
        if int(env.N) != distractor.N:
            raise ValueError(f"the environment steps {env.N} environments, the distractor {distractor.N}")
        if torch.device(env.device) != distractor.device:
            raise ValueError(f"the environment is on {env.device}, the distractor on {distractor.device}")
        self.env, self.distractor = env, distractor
        if distractor.key_from_env and distractor.key is None:
            if not hasattr(env, "background_key"):
                raise ValueError(f"key=\"env\": {type(env).__name__} has no background_key(); give the distractor the clean "
                                 "background image as key=, or key=None for camera and colour alone")
            distractor.set_key(env.background_key())
        self.N, self.A, self.device = env.N, env.A, env.device
        self.episode_length = getattr(env, "episode_length", None)
        self.action_repeat = getattr(env, "action_repeat", 1)
        self._frame = None          # the distracted frames of the newest reset() / step() / render()
        self._images = {}           # (size, channels) -> [buffer, buffer, index of the next]

    @property
    def last_substeps(self):
        return self.env.last_substeps

    def reset(self):
        """env.reset(), and a new episode of the distractions in every environment: the first distracted frames."""
        frame = self.env.reset()
        self.distractor.reset()
        self._frame = self.distractor.apply(frame)
        return self._frame

    def step(self, action):
        """env.step(action) with its frame distracted: (frame, reward, discount, first).  An environment the step reset
        (first = 1) starts a new episode of the distractions with it."""
        frame, reward, discount, first = self.env.step(action)
        self._frame = self.distractor.apply(frame, first)
        return self._frame, reward, discount, first

    def render(self):
        """The current distracted frame again: env.render() and the distractor's render(), which steps no state."""
        self._frame = self.distractor.render(self.env.render())
        return self._frame

    def image(self, size=84, channels=3):
        """The current distracted frames as a renderer hands images out, uint8 [N, size, size, channels]: what the
        built-in tasks' image() is for theirs, two buffers per (size, channels) in turn."""
        size, channels = int(size), int(channels)
        if size not in self.IMAGE_SIZES or channels not in (3, 4):
            raise ValueError(f"image(): size in {self.IMAGE_SIZES} and 3 or 4 channels required, got {size}, {channels}")
        self.distractor._on_gpu()
        if self._frame is None:
            raise _lib.DrqError("image(): call reset() first")
        bufs = self._images.get((size, channels))
        if bufs is None:
            bufs = self._images[size, channels] = [torch.empty((self.N, size, size, channels), dtype=torch.uint8,
                                                               device=self.device) for _ in range(2)] + [0]
        out = bufs[bufs[2]]
        bufs[2] ^= 1
        launch("drq_vec_reach_image", ptr(self._frame), ptr(out), self.N, size, channels, device=self.device)
        return out

    def state(self):
        """env.state() and the distractor's words as "distract_episode" and "distract_t".  This SYNCHRONISES."""
        s = dict(self.env.state())
        s.update({"distract_" + k: v for k, v in self.distractor.state().items()})
        return s

    # ---- checkpoints ---------------------------------------------------------------------
    def state_dict(self):
        """{"format": 1, "kind": "VecDistract", "config": {"N"}, "env": the environment's dict, "distractor": the
        distractor's}.  This SYNCHRONISES, as both of them do."""
        return {"format": 1, "kind": type(self).__name__, "config": {"N": self.N}, "env": self.env.state_dict(),
                "distractor": self.distractor.state_dict()}

    def load_state_dict(self, sd):
        """Restores both parts.  The distractor's part is checked before the environment restores itself, and the
        environment checks its own before it changes, so a mismatch in either names its fields and changes nothing.
        The current distracted frame is drawn again (render()) where the saved environment had been reset."""
        check_state(self, sd, {"N": self.N})
        if not isinstance(sd.get("env"), dict) or not isinstance(sd.get("distractor"), dict):
            raise ValueError("VecDistract.load_state_dict(): the state holds no \"env\" and \"distractor\" parts")
        self.distractor._check(sd["distractor"])
        self.env.load_state_dict(sd["env"])
        self.distractor.load_state_dict(sd["distractor"])
        self._frame = None
        if self.distractor._started and sd["env"].get("reset", True):
            self.render()
