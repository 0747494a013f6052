"""Strong augmentations on the device (new; the reference's only augmentation is its random shift, drqv2.py:19-45, which
here is fused into conv1).

drqv2_amd.distract measures the generalisation gap of a policy; this module holds what closes it.  The two augmentations
every method of DMControl-GB (Hansen & Wang 2021: SVEA, SODA, the "DrQ + aug" baselines) is built from, as one launch each
on a batch of uint8 frame stacks (csrc/strongaug.hip): RandomOverlay blends the observation with an unrelated image
(drq_aug_overlay), RandomConv passes every frame through a random 3 x 3 convolution (drq_aug_random_conv).  Both rules are
spelled out to the bit in include/drqv2_hip.h ("strong augmentation") and restated in numpy by tests/strongaug_oracle.py.
RandomConv is in the image of DMControl-GB's sigmoid(conv2d(x / 255)), not a port of it: the squash is the rational
sigmoid x / (1 + |x|), which numpy reproduces to the bit.  svea_batch() turns either into an SVEA-style update with
DrQV2Agent.update() untouched; noise_bank() makes a bank for callers that have no image set.
"""
import zlib

import torch

from . import _lib
from ._lib import launch, ptr
from .checkpoint import check_state

FRAME_SHAPE = (3, 84, 84)
STACKS = (3, 6, 9, 12)        # the channel counts of a stack of 1 .. 4 RGB frames


class _StrongAug:
    """What the two augmentations share: the generator, the checks of a call, the launch and the state dict.

    aug(obs) takes uint8 [B, C, 84, 84] on the object's device, C in (3, 6, 9, 12) -- a stack of C / 3 RGB frames -- and
    returns a new uint8 tensor of that shape; aug(obs, out=buffer) writes into a contiguous buffer of the caller's.  The
    random numbers of a call are ONE draw from the object's own torch.Generator on its device, so two objects of one seed
    give the same sequence and nothing else in the process moves it.  Every return is written by a launch on the current
    stream; nothing waits for the GPU.  Wrong arguments raise ValueError before anything is drawn or launched; a CPU
    device raises DrqError after those checks.

    state_dict() / load_state_dict() carry "format", "kind", the configuration and the generator's state, so a run that
    augments resumes bit for bit."""

    def __init__(self, device, seed):
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        self.device = torch.device(device)
        self.seed = seed
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(seed)

    def _on_gpu(self):
        if self.device.type != "cuda":
            raise _lib.DrqError("the strong augmentations live on the GPU: the HIP path has no CPU fallback")

    def _tensor(self, t, name, shape=None):
        what = type(self).__name__
        if not torch.is_tensor(t):
            raise ValueError(f"{what}(): {name} must be a tensor on the augmentation's device")
        if shape is None:
            if t.dim() != 4 or t.shape[0] < 1 or t.shape[1] not in STACKS or tuple(t.shape[2:]) != FRAME_SHAPE[1:]:
                raise ValueError(f"{what}(): {name} of shape [B, C, 84, 84] with B >= 1 and C in {STACKS} required, got "
                                 f"{tuple(t.shape)}")
        elif tuple(t.shape) != shape:
            raise ValueError(f"{what}(): {name} of shape {shape} required, got {tuple(t.shape)}")
        if t.dtype != torch.uint8:
            raise ValueError(f"{what}(): {name} must be {torch.uint8}, got {t.dtype}")
        if t.device != _lib.device_index(self.device):
            raise ValueError(f"{what}(): {name} is on {t.device}, the augmentation on {self.device}")
        return t

    def __call__(self, obs, out=None):
        given = self._tensor(obs, "obs")
        if out is not None:
            self._tensor(out, "out", tuple(given.shape))
            if not out.is_contiguous():
                raise ValueError(f"{type(self).__name__}(): out must be contiguous (it is written in place)")
            self._check_out(given, out)
        self._on_gpu()
        obs = given.contiguous()
        with torch.cuda.device(self.device):
            result = torch.empty_like(obs) if out is None else out
            self._launch(obs, result)
            for t in (given, out):      # a caller's tensor may be freed right after the call: the launch still uses it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream())
        return result

    def _check_out(self, obs, out):
        pass

    # ---- checkpoints ---------------------------------------------------------------------
    def state_dict(self):
        """{"format": 1, "kind", "config", "generator"}: the configuration and the generator's state (a uint8 tensor).
        Nothing of the device is read: this does not wait for the GPU."""
        return {"format": 1, "kind": type(self).__name__, "config": self._config(),
                "generator": self.generator.get_state().clone()}

    def load_state_dict(self, sd):
        """Restores what state_dict() saved into an object built with the same arguments: the next call draws what the
        saved object's next call would have drawn.  ValueError, with nothing changed, for a wrong "format" / "kind", a
        configuration that differs (every differing field is named) or a generator state of another size."""
        check_state(self, sd, self._config(), {"generator": self.generator.get_state()})
        self.generator.set_state(sd["generator"].clone())


class RandomOverlay(_StrongAug):
    """
        aug = RandomOverlay(bank, alpha=0.5, device="cuda", seed=0)        # bank: uint8 [M, 3, 84, 84]
        strong = aug(obs)                                                  # uint8 [B, C, 84, 84] -> a new tensor
        aug(obs, out=obs)                                                  # or in place

    Every sample is blended with one image of the bank, the same image over every frame of its stack (as DMControl-GB
    repeats it): out = (obs * (256 - alpha_q8) + image * alpha_q8 + 128) >> 8 in integers, alpha_q8 = int(alpha * 256 +
    0.5).  alpha = 0 returns obs, alpha = 1 the image.  The images are one torch.randint(M, (B,), dtype=int32) draw per
    call from the object's own generator; last_idx keeps them.  The bank (a tensor or an array) is copied to the device
    once; it is configuration: a state dict holds its shape and a CRC of its bytes, not the bytes."""

    def __init__(self, bank, alpha=0.5, device="cuda", seed=0):
        super().__init__(device, seed)
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= alpha <= 1.0:
            raise ValueError(f"alpha must be a number in [0, 1], got {alpha!r}")
        self.alpha_q8 = int(alpha * 256 + 0.5)
        if not torch.is_tensor(bank):
            bank = torch.tensor(bank)          # an array, copied
        if bank.dim() != 4 or bank.shape[0] < 1 or tuple(bank.shape[1:]) != FRAME_SHAPE:
            raise ValueError(f"bank: uint8 [M, 3, 84, 84] with M >= 1 required, got {tuple(bank.shape)}")
        if bank.dtype != torch.uint8:
            raise ValueError(f"bank must be {torch.uint8}, got {bank.dtype}")
        host = bank.detach().to("cpu").contiguous()
        self.bank_crc = zlib.crc32(host.numpy().tobytes())
        self.bank = host.to(self.device, copy=True)
        self.M = int(bank.shape[0])
        self.last_idx = None

    def _launch(self, obs, out):
        B, C = obs.shape[:2]
        self.last_idx = torch.randint(self.M, (B,), dtype=torch.int32, device=self.device, generator=self.generator)
        launch("drq_aug_overlay", ptr(obs), ptr(self.bank), ptr(self.last_idx), ptr(out), B, C, self.M, self.alpha_q8,
               device=self.device)

    def _config(self):
        return {"seed": self.seed, "alpha_q8": self.alpha_q8, "bank_shape": tuple(self.bank.shape), "bank_crc": self.bank_crc}


class RandomConv(_StrongAug):
    """
        aug = RandomConv(device="cuda", seed=0)
        strong = aug(obs)                                                  # uint8 [B, C, 84, 84] -> a new tensor

    Every sample gets a random 3 x 3 convolution of its own, 3 colour channels to 3, applied to each frame of its stack
    with replicate padding and squashed by x / (1 + |x|) into 0 .. 255 (include/drqv2_hip.h has the rule operation by
    operation).  The weights are one torch.randn((B, 3, 3, 3, 3)) draw per call from the object's own generator;
    last_weights keeps them.  The convolution reads neighbours, so out must not share memory with obs."""

    def __init__(self, device="cuda", seed=0):
        super().__init__(device, seed)
        self.last_weights = None

    def _check_out(self, obs, out):
        if out.data_ptr() == obs.data_ptr():
            raise ValueError("RandomConv(): out must not be obs: the convolution reads the neighbours of what it writes")

    def _launch(self, obs, out):
        B, C = obs.shape[:2]
        self.last_weights = torch.randn((B, 3, 3, 3, 3), dtype=torch.float32, device=self.device, generator=self.generator)
        launch("drq_aug_random_conv", ptr(obs), ptr(self.last_weights), ptr(out), B, C, device=self.device)

    def _config(self):
        return {"seed": self.seed}


def noise_bank(M, seed=0, device="cpu", grid=6):
    """A bank for RandomOverlay made from nothing: M images uint8 [M, 3, 84, 84], each a random RGB grid of grid x grid
    points upsampled bilinearly to 84 x 84 -- smooth colour blobs, for users and tools that have no image set.  Plain
    torch on the host (its own generator of `seed`), then moved to `device`; not pinned to the bit across torch versions."""
    M, grid = int(M), int(grid)
    if M < 1 or grid < 2:
        raise ValueError(f"noise_bank(): M >= 1 images of a grid >= 2 required, got {M}, {grid}")
    g = torch.Generator()
    g.manual_seed(int(seed))
    low = torch.rand((M, 3, grid, grid), generator=g)
    img = torch.nn.functional.interpolate(low, size=FRAME_SHAPE[1:], mode="bilinear", align_corners=True)
    return (img * 255.0 + 0.5).clamp_(0, 255).to(torch.uint8).to(device)


def svea_batch(batch, strong):
    """The batch of an SVEA-style update (Hansen, Su & Wang 2021) from a materialised one.

        batch = svea_batch(store_batch.materialize(), strong)          # strong: a RandomOverlay or RandomConv, or any
        agent.update(iter([batch]), step)                               # callable uint8 [B, C, 84, 84] -> the same

    batch is the 5-tuple (obs, action, reward, discount, next_obs) of tensors with B rows; the return is the 2B-row tuple
    (cat(obs, strong(obs)), action x 2, reward x 2, discount x 2, next_obs x 2).  Fed to the unchanged update(), the
    critic loss is the mean over both halves against one target per transition: SVEA's objective with alpha = beta = 0.5.
    next_obs, and so the target, never sees the strong augmentation.  strong is called exactly once.

    Two differences from the paper, both because update() is untouched: the actor step also sees the augmented half
    (SVEA trains the actor on clean observations only), and the two halves get independent random shifts, because the
    shift is drawn inside update() per row (SVEA applies the strong augmentation on top of one shifted view)."""
    obs, action, reward, discount, next_obs = batch
    twice = lambda t: torch.cat((t, t), dim=0)
    return (torch.cat((obs, strong(obs)), dim=0), twice(action), twice(reward), twice(discount), twice(next_obs))
