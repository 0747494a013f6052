"""Built-in device environments for vectorised collection (new; the reference steps one dm_control environment on the
host, dmc.py / train.py:160-190).

VecReach is the producer the device-side collection path was missing: N lockstep environments of a small pixel task
("reach": a point in a square must reach a target) stepped by ONE launch (csrc/vecenv.hip, drq_vec_task_step) that writes
what VecFrameReplay.add(), add_render() and VecEpisodeStats.step() take -- uint8 [N, 3, 84, 84] frames, reward, discount
and first -- as device tensors on the current stream.  VecPointMass is the same square with momentum: the action
accelerates the point, and its velocity is in no single frame, so it is the one task here that needs the three-frame
stack.  Both take action_repeat (the ActionRepeatWrapper of dmc.py:35-50, inside the launch).  The tasks are specified to
the bit in include/drqv2_hip.h ("device environment") and restated in numpy by tests/vec_env_oracle.py and
tests/vec_tasks_oracle.py.  They are not benchmark tasks and say nothing about DMC.

VecCartpole is a third task with a kernel of its own (csrc/veccartpole.hip, drq_vec_cartpole_step): a cart on a rail that
carries a free pole, started hanging or near upright, in the image of the reference's cartpole_swingup and
cartpole_balance (cfgs/task/easy.yaml) -- an action that acts through second-order coupled dynamics and an unstable
equilibrium.  It shares _VecTask with the other two; what differs per task -- the entries, the state arrays and their
arguments -- are _VecTask's hooks.  Specified in include/drqv2_hip.h ("Cartpole"), restated by tests/vec_cartpole_oracle.py.

VecReacher is a fourth (csrc/vecreacher.hip, drq_vec_reacher_step): a planar two-link arm driven by torques at the
shoulder and the elbow, in the image of the reference's reacher_easy and reacher_hard -- the one task here with a sparse
reward, 1 while the fingertip is inside the target disc and 0 otherwise, which is what the exploration bonus, the
demonstrations, prioritized replay and the DrM blocks are for.  Specified in include/drqv2_hip.h ("Reacher"), restated by
tests/vec_reacher_oracle.py.

VecMaze is a fifth (csrc/vecmaze.hip, drq_vec_maze_step): a point in a square that walls cut into size x size cells must find
the goal cell.  The walls are generated on the device at every reset -- a binary-tree maze put through one of the 8
symmetries of the square, with loops opened on request -- fresh per episode or from a finite pool of `layouts` mazes that
`layout_seed` names, so a user trains on K layouts and evaluates on others.  The reward sits behind walls: it is the task
the exploration bonuses are for, and the one whose dynamics differ between episodes.  Specified in include/drqv2_hip.h
("Maze"), restated by tests/vec_maze_oracle.py.

VecCatch is a sixth (csrc/veccatch.hip, drq_vec_catch_step): a cup driven in the plane, a ball tied to it by a string that is
either slack or taut, and three capsules that the ball collides with, in the image of the reference's cup_catch
(cfgs/task/cup_catch.yaml) -- the one task here with a unilateral constraint, contacts between moving bodies and dynamics
that switch regime inside an episode, and a sparse reward that needs a timed sequence: swing the ball up, then get the cup
under it.  Specified in include/drqv2_hip.h ("Catch"), restated by tests/vec_catch_oracle.py, which also holds a scripted
controller that solves it.

VecWalker is a seventh (csrc/vecwalker.hip, drq_vec_walker_step): a planar legged runner of six particles and five rods
under position-based dynamics, with four muscles and a ground with friction, in the image of the reference's walker_stand,
walker_walk, walker_run and cheetah_run -- the one locomotion task here: ground contact, four actuators, an unbounded
coordinate that the camera follows, and a reward on speed.  Specified in include/drqv2_hip.h ("Walker"), restated by
tests/vec_walker_oracle.py, which also holds a scripted open-loop gait that makes it run.

VecFinger is an eighth (csrc/vecfinger.hip, drq_vec_finger_step): the reacher's arm above a rod that turns freely on a hinge,
in the image of the reference's finger_spin, finger_turn_easy and finger_turn_hard -- the one manipulation task here: the
agent drives one body and is paid for the motion of another, which it can only influence through contact.  Specified in
include/drqv2_hip.h ("Finger"), restated by tests/vec_finger_oracle.py, which also holds a scripted controller per mode.
"""
import torch

from . import _lib
from ._lib import launch, ptr
from .checkpoint import check_state, host


MAX_ACTION_REPEAT = 16        # DRQ_TASK_MAX_REPEAT


class _VecTask:
    """What the device environments share: everything but the task's name, its id in the library and its state arrays.

        env = VecReach(num_envs=N, device="cuda", action_dim=A, episode_length=250, seed=0, action_repeat=1)
        frame = env.reset()                                   # uint8 [N, 3, 84, 84]
        frame, reward, discount, first = env.step(action)     # action float32 [N, A] on the device

    action_repeat = K (1 .. 16) makes step() a macro step of up to K simulator steps under the one action, inside the
    launch: reward = sum of r_i times the running product of the discounts before it, discount = their product, and an
    environment whose episode ends inside the repeat stops there (dmc.py:40-50).  t and episode_length count simulator
    steps, as in DMC; a row of the ring or of VecEpisodeStats is one step() call.  last_substeps is the int32 [N] device
    tensor of the simulator steps the newest step() / reset() took per environment (0 on a reset row), from the same two
    rotating output sets as the rest.

    Per environment: pos and target in [-1, 1]^2, t (steps of this episode), episode (a counter), over (the last step
    ended the episode).  A simulator step of reach (VecPointMass states its own) moves pos by clamp(action[:, :2], -1, 1)
    * 0.1 (NaN counts as 0; further columns are ignored), reward = max(0, 1 - |pos - target|^2); |pos - target|^2 <= 0.01
    ends the episode with discount 0 (reached), t == episode_length with discount 1 (the time limit).  The step() AFTER one
    that ended the episode is the reset row
    of that environment: first = 1, reward 0, discount 1, the first frame of a new episode whose positions are a hash of
    (seed, environment, episode); its action is ignored.  So resets are staggered across the environments, as the rings
    and the statistics expect them.  Everything is deterministic to the bit for a seed and a sequence of actions.

    Every return is a device tensor written by a launch on the current stream; nothing waits for the GPU.  step() and
    reset() write into TWO output sets (frame, reward, discount, first, substeps) used in turn, as VecFrameReplay.observation()
    does: a returned tensor is overwritten by the second step() / reset() / render() call after it, so a caller that
    keeps one longer clones it.  image() rotates two buffers per (size, channels) in the same way.

    Checkpoints: state_dict() / load_state_dict() save and restore the state words of every environment (seven for
    reach, nine with the point mass's velocity); the frames are derived data and are drawn again from the restored state
    (render(): drq_vec_reach_render, one launch)."""

    FRAME_SHAPE = (3, 84, 84)
    IMAGE_SIZES = (84, 168, 252, 336)
    TASK = TASK_ID = None       # the name in state dicts and tools; DRQ_TASK_* of include/drqv2_hip.h
    _STATE = ("pos", "target", "t", "episode", "over")      # the state arrays, in the order of state() and state_dict()
    _STATE_SPEC = {"pos": ((2,), torch.float32), "target": ((2,), torch.float32), "vel": ((2,), torch.float32),
                   "t": ((), torch.int32), "episode": ((), torch.int32), "over": ((), torch.uint8)}
    _MIN_ACTION_DIM = 2         # the columns of the action a step reads
    vel = None                  # reach has no velocity: the library is handed NULL

    def __init__(self, num_envs, device, action_dim=2, episode_length=250, seed=0, action_repeat=1):
        if isinstance(action_repeat, bool) or not isinstance(action_repeat, int) \
                or not 1 <= action_repeat <= MAX_ACTION_REPEAT:
            raise ValueError(f"action_repeat must be an int in 1 .. {MAX_ACTION_REPEAT}, got {action_repeat!r}")
        self.action_repeat = action_repeat
        self.N, self.A, self.episode_length = int(num_envs), int(action_dim), int(episode_length)
        if self.N < 1 or self.A < self._MIN_ACTION_DIM or self.episode_length < 1:
            raise ValueError(f"num_envs and episode_length must be >= 1, action_dim >= {self._MIN_ACTION_DIM}")
        self.seed = int(seed) & 0xFFFFFFFF
        self.device = dev = torch.device(device)
        for k in self._STATE:       # episode is uint32 on the device: state() views it so
            shape, dtype = self._STATE_SPEC[k]
            setattr(self, k, torch.zeros((self.N,) + shape, dtype=dtype, device=dev))
        self.last_substeps = None   # int32 [N] of the newest step() / reset()
        self._out = None            # two of (frame, reward, discount, first, substeps), then the index of the next
        self._frame = None          # the frames of the newest step() / reset()
        self._images = {}           # (size, channels) -> [buffer, buffer, index of the next]

    def _on_gpu(self):
        if self.device.type != "cuda":
            raise _lib.DrqError("the device environment lives on the GPU: the HIP path has no CPU fallback")

    def _action(self, action):
        N, A = self.N, self.A
        if not torch.is_tensor(action):
            raise ValueError("step(): action must be a tensor on the environment's device")
        if tuple(action.shape) != (N, A):
            raise ValueError(f"step(): action of shape {(N, A)} required, got {tuple(action.shape)}")
        if action.dtype != torch.float32:
            raise ValueError(f"step(): action must be {torch.float32}, got {action.dtype}")
        if action.device != _lib.device_index(self.device):
            raise ValueError(f"step(): action is on {action.device}, the environment on {self.device}")
        return action.contiguous()

    def _next_out(self):
        """the output set (frame, reward, discount, first, substeps) the next launch writes"""
        if self._out is None:
            dev, N = self.device, self.N
            self._out = [(torch.empty((N,) + self.FRAME_SHAPE, dtype=torch.uint8, device=dev),
                          torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                          torch.empty(N, dtype=torch.uint8, device=dev),
                          torch.empty(N, dtype=torch.int32, device=dev)) for _ in range(2)] + [0]
        out = self._out[self._out[2]]
        self._out[2] ^= 1
        return out

    def _launch(self, action, reset_all):
        out = self._next_out()
        with torch.cuda.device(self.device):
            self._step_launch(action, reset_all, out)
            if action is not None:  # a caller's tensor may be freed right after step(): the launch still reads it
                action.record_stream(torch.cuda.current_stream())
        self._frame, self.last_substeps = out[0], out[4]
        return out[:4]

    def _step_launch(self, action, reset_all, out):
        """the task's step entry: the macro step (or the reset of all) of every environment into the output set `out`"""
        launch("drq_vec_task_step", self.TASK_ID, ptr(self.pos), ptr(self.target), ptr(self.vel), ptr(self.t),
               ptr(self.episode), ptr(self.over), self.N, self.A, ptr(action), self.seed, self.episode_length,
               self.action_repeat, int(reset_all), *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        """the task's render entry: the frames of the states as they are into `frame`"""
        launch("drq_vec_reach_render", ptr(self.pos), ptr(self.target), self.N, ptr(frame), device=self.device)

    def reset(self):
        """Starts a new episode in every environment (one launch) and returns its first frames, uint8 [N, 3, 84, 84].  The
        row is a reset row for every environment: what goes into the ring beside it is add(frame, zeros, zeros, ones)."""
        self._on_gpu()
        return self._launch(None, True)[0]

    def step(self, action):
        """action: float32 [N, action_dim] tensor on the environment's device (what agent.act_batch() returns); ValueError
        otherwise.  One launch; returns (frame uint8 [N, 3, 84, 84], reward float32 [N], discount float32 [N], first
        uint8 [N]) from one of the two output sets used in turn.  An environment whose previous step ended its episode is
        reset by this call: first = 1, the frame is the new episode's first, reward = 0 and discount = 1 are dummies."""
        action = self._action(action)
        self._on_gpu()
        if self._frame is None:
            raise _lib.DrqError("step(): call reset() first")
        return self._launch(action, False)

    def render(self):
        """The frames of the current state, uint8 [N, 3, 84, 84]: one launch (drq_vec_reach_render) that reads pos and
        target and changes no state.  After reset() or step() it returns exactly the frame they returned; after
        load_state_dict() it is how the restored environment gets its frames.  It writes into the next of the two output
        sets, like step(), and that frame becomes the one image() reads."""
        self._on_gpu()
        if self._frame is None:
            raise _lib.DrqError("render(): call reset() or load_state_dict() first")
        return self._render()

    def _render(self):
        out = self._next_out()
        self._render_launch(out[0])
        self._frame = out[0]
        return out[0]

    def image(self, size=84, channels=3):
        """The current frames as a renderer hands images out: uint8 [N, size, size, channels], channels last, size 84,
        168, 252 or 336 (every pixel size / 84 times in both directions), channels 3 or 4 (the fourth is 255).  One
        launch (drq_vec_reach_image); VecFrameReplay.add_render() of it stores exactly the frame."""
        size, channels = int(size), int(channels)
        if size not in self.IMAGE_SIZES or channels not in (3, 4):
            raise ValueError(f"image(): size in {self.IMAGE_SIZES} and 3 or 4 channels required, got {size}, {channels}")
        self._on_gpu()
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

    def background_key(self):
        """The background every task here draws behind its shapes, uint8 [3, 84, 84] on the environment's device: the
        ramp 32 + ((i + j) >> 2) in all three channels (include/drqv2_hip.h, "device environment").  It is the `key` of
        drqv2_amd.distract.FrameDistractor: a pixel of a frame that equals it is background."""
        i = torch.arange(84, device=self.device)
        ramp = (32 + ((i[:, None] + i[None, :]) >> 2)).to(torch.uint8)
        return ramp.expand(self.FRAME_SHAPE).contiguous()

    def state(self):
        """Host copies of the state, for tests and debugging: {"pos": float32 [N, 2], "target": float32 [N, 2], "t": int32
        [N], "episode": uint32 [N], "over": uint8 [N]}, and "vel": float32 [N, 2] for the point mass.  This SYNCHRONISES:
        the copies wait for every launch enqueued so far.  Nothing in a collection loop should call it."""
        import numpy as np
        s = {k: getattr(self, k).cpu().numpy() for k in self._STATE}
        s["episode"] = s["episode"].view(np.uint32)
        return s

    # ---- checkpoints ---------------------------------------------------------------------
    def _config(self):
        return {"N": self.N, "A": self.A, "episode_length": self.episode_length, "seed": self.seed, "task": self.TASK,
                "action_repeat": self.action_repeat}

    def state_dict(self):
        """The environment as a plain dict of CPU tensors and Python scalars: "format": 1, "kind", the configuration (N,
        A, episode_length, seed, task, action_repeat) and the state words per environment (pos, target, t, episode, over,
        and vel for the point mass; episode as the int32 tensor that holds its uint32 bits).  The newest frames are not
        in it: they are a function of the state.  This SYNCHRONISES the environment's device, like state(): the copies
        wait for every launch enqueued so far."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        sd = {"format": 1, "kind": type(self).__name__, "reset": self._frame is not None, "config": self._config()}
        for k in self._STATE:
            sd[k] = host(getattr(self, k))
        return sd

    def load_state_dict(self, sd):
        """Restores what state_dict() saved, into a fresh or a used environment.  ValueError, with nothing changed, for a
        wrong "format" / "kind" or a configuration that differs from this object's (every differing field is named, the
        task and action_repeat among them).  A VecReach dict written before there were tasks has neither key and is read
        as task "reach", action_repeat 1.  The frames are drawn from the restored state with one launch (render()'s), so
        step() and image() work without a reset() -- unless the saved environment had never been reset.  DrqError on a
        CPU device, after the checks."""
        if isinstance(sd, dict) and isinstance(sd.get("config"), dict) and sd.get("kind") == "VecReach":
            sd = dict(sd, config=dict({"task": "reach", "action_repeat": 1}, **sd["config"]))
        check_state(self, sd, self._config(), {k: getattr(self, k) for k in self._STATE})
        self._on_gpu()
        for k in self._STATE:
            getattr(self, k).copy_(sd[k])
        self._frame = None
        if sd.get("reset", True):
            self._render()


class VecReach(_VecTask):
    """N environments of the reach task on the device: the action moves the point, touching the target ends the episode
    (_VecTask holds the interface and the rules)."""
    TASK, TASK_ID = "reach", 0


class VecPointMass(_VecTask):
    """N environments of the point-mass task on the device: the reach square with momentum.  Per axis and simulator step
    vel = vel * 0.9 + a * 0.02 and pos += vel; a wall stops the axis that hits it (pos = +-1, vel = 0).  The reward is
    reach's, max(0, 1 - |pos - target|^2); touching the target does NOT end the episode: discount is 1 on every row and
    only the time limit ends one.  Resets draw pos and target as reach does and set vel = 0.  The velocity is in no
    frame -- two states that differ only in vel look alike -- so the policy needs the frame stack.  Same constructor and
    methods as VecReach; state() and state_dict() carry "vel" too."""
    TASK, TASK_ID = "pointmass", 1
    _STATE = _VecTask._STATE + ("vel",)


class VecCartpole(_VecTask):
    """N environments of the cartpole on the device: a cart on a rail carries a free pole, and action[:, 0] in [-1, 1]
    pushes the cart with a force of 10 (NaN counts as 0; further columns are ignored).  swing_up=True starts every
    episode with the pole hanging down (the reference's cartpole_swingup), swing_up=False with it near upright
    (cartpole_balance): the first task here whose action acts through second-order coupled dynamics, with an unstable
    equilibrium.  It is a task in the image of those two, not a port of them: the frictionless textbook equations
    stepped by semi-implicit Euler at dt = 0.01, the pole's angle held as a unit vector so that a step is +, -, *, / and
    sqrt alone, and DMC's reward product with rational sigmoids -- upright (c + 1) / 2, centred, small control, small
    angular velocity, each in [0, 1].  Nothing it scores says anything about DMC.  The rule is in include/drqv2_hip.h
    ("Cartpole") to the bit and restated in numpy by tests/vec_cartpole_oracle.py.

        env = VecCartpole(num_envs=N, device="cuda", action_dim=1, episode_length=1000, seed=0, action_repeat=1,
                          swing_up=True)

    The discount is 1 on every row and only the time limit (t == episode_length, in simulator steps) ends an episode; the
    rail ends at x = +-1.8 stop the cart as the point mass's walls do.  The frame shows the rail (blue), the cart (green)
    and the pole (red, a capsule) at 20 pixels per unit, so the whole pole is in the picture for |x| <= 0.9; neither
    velocity is in a frame, so the policy needs the frame stack.  Same methods and guarantees as VecReach (_VecTask
    holds them): reset, step, render, image, state, state_dict, load_state_dict and last_substeps, two rotating output
    sets, nothing waits for the GPU.  The state words are "phys", float32 [N, 5] = (x, xdot, cos, sin, omega), and t,
    episode, over; the config of a state dict carries swing_up."""
    TASK = "cartpole"
    _STATE = ("phys", "t", "episode", "over")
    _STATE_SPEC = dict(_VecTask._STATE_SPEC, phys=((5,), torch.float32))
    _MIN_ACTION_DIM = 1

    def __init__(self, num_envs, device, action_dim=1, episode_length=1000, seed=0, action_repeat=1, swing_up=True):
        if not isinstance(swing_up, (bool, int)) or swing_up not in (0, 1):
            raise ValueError(f"swing_up must be True or False, got {swing_up!r}")
        self.swing_up = bool(swing_up)
        super().__init__(num_envs, device, action_dim, episode_length, seed, action_repeat)

    def _step_launch(self, action, reset_all, out):
        launch("drq_vec_cartpole_step", ptr(self.phys), ptr(self.t), ptr(self.episode), ptr(self.over), self.N, self.A,
               ptr(action), self.seed, self.episode_length, self.action_repeat, int(reset_all), int(self.swing_up),
               *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        launch("drq_vec_cartpole_render", ptr(self.phys), self.N, ptr(frame), device=self.device)

    def _config(self):
        return dict(super()._config(), swing_up=self.swing_up)


class VecReacher(_VecTask):
    """N environments of the reacher on the device: a planar arm of two links of 0.5, seen from above (no gravity), with
    a point mass of 1 at the elbow and one at the fingertip.  action[:, 0] in [-1, 1] is the torque at the shoulder and
    action[:, 1] the torque at the elbow, each times 2 (NaN counts as 0; further columns are ignored); both joints are
    damped, coupled through the full inertia matrix and its Coriolis terms, and have no limits.  sparse=True pays 1 for
    every simulator step whose fingertip is inside the target disc of radius target_radius and 0 otherwise: about 0.15 is
    the reference's reacher_easy, about 0.05 its reacher_hard.  sparse=False pays 1 / (1 + 4 d^2) of the distance d
    between fingertip and target instead: a dense shaping of the same geometry, for debugging and as the comparison arm
    of a demo.  It is a task in the image of those two, not a port of them, and nothing it scores says anything about
    DMC.  The rule is in include/drqv2_hip.h ("Reacher") to the bit and restated in numpy by tests/vec_reacher_oracle.py.

        env = VecReacher(num_envs=N, device="cuda", action_dim=2, episode_length=1000, seed=0, action_repeat=1,
                         target_radius=0.15, sparse=True)

    The discount is 1 on every row and only the time limit (t == episode_length, in simulator steps) ends an episode, so
    a macro step's sparse reward is an exact small integer.  A reset draws both joint angles and a target whose whole
    disc the fingertip can cover.  The frame shows the target (green), the upper arm (blue), the forearm (red) and the
    fingertip (yellow) at 36 pixels per unit, the shoulder in the middle; neither velocity is in a frame, so the policy
    needs the frame stack.  Same methods and guarantees as VecReach (_VecTask holds them).  The state words are "phys",
    float32 [N, 6] = (c1, s1, w1, c2, s2, w2) -- the shoulder's unit vector, the elbow's relative to the upper arm, the
    angular velocities -- "target", float32 [N, 2], and t, episode, over; the config of a state dict carries
    target_radius and sparse."""
    TASK = "reacher"
    _STATE = ("phys", "target", "t", "episode", "over")
    _STATE_SPEC = dict(_VecTask._STATE_SPEC, phys=((6,), torch.float32))
    MIN_TARGET_RADIUS, MAX_TARGET_RADIUS = 0.02, 0.3

    def __init__(self, num_envs, device, action_dim=2, episode_length=1000, seed=0, action_repeat=1, target_radius=0.15,
                 sparse=True):
        if isinstance(target_radius, bool) or not isinstance(target_radius, (int, float)) \
                or not self.MIN_TARGET_RADIUS <= target_radius <= self.MAX_TARGET_RADIUS:
            raise ValueError(f"target_radius must be a number in {self.MIN_TARGET_RADIUS} .. {self.MAX_TARGET_RADIUS}, "
                             f"got {target_radius!r}")
        if not isinstance(sparse, (bool, int)) or sparse not in (0, 1):
            raise ValueError(f"sparse must be True or False, got {sparse!r}")
        self.target_radius, self.sparse = float(target_radius), bool(sparse)
        super().__init__(num_envs, device, action_dim, episode_length, seed, action_repeat)

    def _step_launch(self, action, reset_all, out):
        launch("drq_vec_reacher_step", ptr(self.phys), ptr(self.target), ptr(self.t), ptr(self.episode), ptr(self.over),
               self.N, self.A, ptr(action), self.seed, self.episode_length, self.action_repeat, int(reset_all),
               self.target_radius, int(self.sparse), *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        launch("drq_vec_reacher_render", ptr(self.phys), ptr(self.target), self.N, self.target_radius, ptr(frame),
               device=self.device)

    def _config(self):
        return dict(super()._config(), target_radius=self.target_radius, sparse=self.sparse)


class VecCatch(_VecTask):
    """N environments of the catch on the device: in the world [-1, 1]^2 with gravity 4 along -y a cup -- a floor of width
    cup_width and two walls of height 0.15, three capsules of radius 0.02 -- is driven by action[:, 0:2] in [-1, 1] per
    axis with momentum, as the point mass is (v = v * 0.9 + a * 0.3, at most 1.5; a stop at +-0.4 zeroes the axis; NaN
    counts as 0; further columns are ignored).  A ball of radius 0.05 hangs from the middle of the cup's inside floor on a
    tether of length 0.5: inside that length the string is slack and the ball flies free, at that length it is pulled
    back inelastically; the ball collides with the three capsules without restitution.  sparse=True pays 1 for every
    simulator step whose ball centre is inside the cup -- between the walls, above the floor, below the rim -- and 0
    otherwise; sparse=False pays 1 / (1 + 4 d^2) of the distance d between the ball and the middle of the cup's interior
    instead, the reacher's shaping.  cup_width is the difficulty: 0.3 leaves the ball of diameter 0.1 an opening of 0.26,
    0.18 one of 0.14.  It is a task in the image of DMC's ball-in-cup (the reference's cup_catch), not a port of it, and
    nothing it scores says anything about DMC.  The rule is in include/drqv2_hip.h ("Catch") to the bit and restated in
    numpy by tests/vec_catch_oracle.py, whose expert() swings the ball up and catches it.

        env = VecCatch(num_envs=N, device="cuda", action_dim=2, episode_length=1000, seed=0, action_repeat=1,
                       cup_width=0.3, sparse=True)

    The discount is 1 on every row and only the time limit (t == episode_length, in simulator steps) ends an episode, so
    a macro step's sparse reward is an exact small integer.  A reset draws the cup's position and hangs the ball at rest
    at the tether's length, a little off the vertical.  The frame is the world at 42 pixels per unit: the tether (cyan),
    the left wall (blue), the right wall (magenta), the floor (green) and the ball (yellow); no velocity is in a frame, so
    the policy needs the frame stack.  Same methods and guarantees as VecReach (_VecTask holds them).  The state words are
    "phys", float32 [N, 8] = (cx, cy, vcx, vcy, bx, by, vbx, vby) -- the cup's position and velocity, the ball's -- and t,
    episode, over; the config of a state dict carries cup_width and sparse."""
    TASK = "catch"
    _STATE = ("phys", "t", "episode", "over")
    _STATE_SPEC = dict(_VecTask._STATE_SPEC, phys=((8,), torch.float32))
    MIN_CUP_WIDTH, MAX_CUP_WIDTH = 0.16, 0.4

    def __init__(self, num_envs, device, action_dim=2, episode_length=1000, seed=0, action_repeat=1, cup_width=0.3,
                 sparse=True):
        if isinstance(cup_width, bool) or not isinstance(cup_width, (int, float)) \
                or not self.MIN_CUP_WIDTH <= cup_width <= self.MAX_CUP_WIDTH:
            raise ValueError(f"cup_width must be a number in {self.MIN_CUP_WIDTH} .. {self.MAX_CUP_WIDTH}, got {cup_width!r}")
        if not isinstance(sparse, (bool, int)) or sparse not in (0, 1):
            raise ValueError(f"sparse must be True or False, got {sparse!r}")
        self.cup_width, self.sparse = float(cup_width), bool(sparse)
        super().__init__(num_envs, device, action_dim, episode_length, seed, action_repeat)

    def _step_launch(self, action, reset_all, out):
        launch("drq_vec_catch_step", ptr(self.phys), ptr(self.t), ptr(self.episode), ptr(self.over), self.N, self.A,
               ptr(action), self.seed, self.episode_length, self.action_repeat, int(reset_all), self.cup_width,
               int(self.sparse), *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        launch("drq_vec_catch_render", ptr(self.phys), self.N, self.cup_width, ptr(frame), device=self.device)

    def _config(self):
        return dict(super()._config(), cup_width=self.cup_width, sparse=self.sparse)


class VecWalker(_VecTask):
    """N environments of the walker on the device: a planar legged runner above a ground at y = 0 with gravity 10 along
    -y, in a world that is unbounded in x (periodic with period 4).  The body is six unit point masses -- shoulder, hip,
    front knee, front foot, back knee, back foot -- held by five rigid rods (a torso of 0.4 with a leg of two limbs of
    0.25 at either end) under position-based dynamics.  action[:, 0:4] in [-1, 1] sets the target lengths of four muscles,
    each a distance across a joint: front hip, front knee, back hip, back knee (NaN counts as 0; further columns are
    ignored).  A muscle closes half its error per sweep up to a force limit; hard limits on the same distances keep every
    joint away from straight and from folded.  The ground stops a particle at y = 0 and leaves it a tenth of its
    horizontal velocity, which is the friction the body pushes on.  speed = 0 pays stand, the torso's height (0 at 0.1,
    1 from 0.2) times its uprightness; speed > 0 pays stand * (1 + 5 * move) / 6 with move = clamp(v / speed, 0, 1) of the
    torso's forward velocity, the form of DMC's walker.  WALK_SPEED is about what a scripted open-loop gait reaches,
    RUN_SPEED twice that.  It is a task in the image of DMC's walker and cheetah (the reference's walker_stand,
    walker_walk, walker_run and cheetah_run), not a port of them, and nothing it scores says anything about DMC.  The
    rule is in include/drqv2_hip.h ("Walker") to the bit and restated in numpy by tests/vec_walker_oracle.py, whose gait()
    makes the body run.

        env = VecWalker(num_envs=N, device="cuda", action_dim=4, episode_length=1000, seed=0, action_repeat=1, speed=0.3)

    The discount is 1 on every row and only the time limit (t == episode_length, in simulator steps) ends an episode: a
    fallen body lies there until then.  A reset draws a standing pose, the torso a little tilted.  The camera follows the
    torso's middle at 42 pixels per unit: the ramp background stays fixed to the frame, the ground is a band of green and
    blue stripes fixed to the world, the back leg is magenta, the torso red, the front leg cyan; no velocity is in a
    frame -- it shows in how the ground scrolls -- so the policy needs the frame stack.  Same methods and guarantees as
    VecReach (_VecTask holds them).  The state words are "phys", float32 [N, 24] = (x, y, vx, vy) of each of the six
    particles, and t, episode, over; the config of a state dict carries speed."""
    TASK = "walker"
    _MIN_ACTION_DIM = 4
    _STATE = ("phys", "t", "episode", "over")
    _STATE_SPEC = dict(_VecTask._STATE_SPEC, phys=((24,), torch.float32))
    MAX_SPEED, WALK_SPEED, RUN_SPEED = 2.0, 0.3, 0.6

    def __init__(self, num_envs, device, action_dim=4, episode_length=1000, seed=0, action_repeat=1, speed=WALK_SPEED):
        if isinstance(speed, bool) or not isinstance(speed, (int, float)) or not 0 <= speed <= self.MAX_SPEED:
            raise ValueError(f"speed must be a number in 0 .. {self.MAX_SPEED}, got {speed!r}")
        self.speed = float(speed)
        super().__init__(num_envs, device, action_dim, episode_length, seed, action_repeat)

    def _step_launch(self, action, reset_all, out):
        launch("drq_vec_walker_step", ptr(self.phys), ptr(self.t), ptr(self.episode), ptr(self.over), self.N, self.A,
               ptr(action), self.seed, self.episode_length, self.action_repeat, int(reset_all), self.speed,
               *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        launch("drq_vec_walker_render", ptr(self.phys), self.N, ptr(frame), device=self.device)

    def _config(self):
        return dict(super()._config(), speed=self.speed)


class VecFinger(_VecTask):
    """N environments of the finger on the device: in the world [-1, 1]^2 without gravity a finger -- the reacher's arm, links
    of 0.4 and 0.3 rooted at (0, 0.2), a fingertip disc of radius 0.06 -- hangs above a spinner, a rod of length 0.3 and
    radius 0.05 that turns freely on a hinge at (0, -0.2) and loses 3 % of its angular velocity per simulator step.
    action[:, 0] in [-1, 1] is the torque at the shoulder and action[:, 1] the torque at the elbow, each times 2 (NaN counts
    as 0; further columns are ignored).  Only the fingertip collides, and only with the rod, without restitution: the
    agent is paid for the motion of a body it can only push.  task="spin" pays 1 for every simulator step on which the rod
    turns anticlockwise at SPIN_SPEED or faster (sparse=False: clamp(ws / SPIN_SPEED, 0, 1)); a velocity, so it shows
    only across stacked frames.  task="turn" pays 1 while the rod's tip is inside a target disc of radius target_radius
    centred on the rod's circle (sparse=False: 1 / (1 + 4 d^2) of the distance d between the two, the reacher's shaping):
    TURN_EASY_RADIUS and TURN_HARD_RADIUS are the reference's finger_turn_easy and finger_turn_hard.  It is a task in the
    image of DMC's finger, not a port of it, and nothing it scores says anything about DMC.  The rule is in
    include/drqv2_hip.h ("Finger") to the bit and restated in numpy by tests/vec_finger_oracle.py, whose flick() and
    turn_to() solve the two modes.

        env = VecFinger(num_envs=N, device="cuda", action_dim=2, episode_length=1000, seed=0, action_repeat=1,
                        task="spin", target_radius=VecFinger.TURN_EASY_RADIUS, sparse=True)

    The discount is 1 on every row and only the time limit (t == episode_length, in simulator steps) ends an episode, so
    a macro step's sparse reward is an exact small integer.  A reset draws both joint angles, the rod's angle and a
    target angle at least 45 degrees from the rod's; no episode starts in contact.  The frame is the world at 42 pixels per
    unit: the target (green, turn only), the hinge and the rod's tip (blue), the rod (magenta), the upper link (red), the
    forearm (cyan) and the fingertip (yellow); no velocity is in a frame, so the policy needs the frame stack.  Same
    methods and guarantees as VecReach (_VecTask holds them).  The state words are "phys", float32 [N, 9] = (c1, s1, w1,
    c2, s2, w2, cs, ss, ws) -- the shoulder's unit vector and angular velocity, the elbow's, the rod's -- "target", float32
    [N, 2], the unit vector of the target's angle (drawn in both modes), and t, episode, over; the config of a state dict
    carries mode, target_radius and sparse."""
    TASK = "finger"
    _STATE = ("phys", "target", "t", "episode", "over")
    _STATE_SPEC = dict(_VecTask._STATE_SPEC, phys=((9,), torch.float32))
    MODES = ("spin", "turn")
    MIN_TARGET_RADIUS, MAX_TARGET_RADIUS = 0.02, 0.2
    TURN_EASY_RADIUS, TURN_HARD_RADIUS, SPIN_SPEED = 0.1, 0.04, 2.0

    def __init__(self, num_envs, device, action_dim=2, episode_length=1000, seed=0, action_repeat=1, task="spin",
                 target_radius=TURN_EASY_RADIUS, sparse=True):
        if not isinstance(task, str) or task not in self.MODES:
            raise ValueError(f"task must be one of {self.MODES}, got {task!r}")
        if isinstance(target_radius, bool) or not isinstance(target_radius, (int, float)) \
                or not self.MIN_TARGET_RADIUS <= target_radius <= self.MAX_TARGET_RADIUS:
            raise ValueError(f"target_radius must be a number in {self.MIN_TARGET_RADIUS} .. {self.MAX_TARGET_RADIUS}, "
                             f"got {target_radius!r}")
        if not isinstance(sparse, (bool, int)) or sparse not in (0, 1):
            raise ValueError(f"sparse must be True or False, got {sparse!r}")
        self.mode, self.target_radius, self.sparse = task, float(target_radius), bool(sparse)
        super().__init__(num_envs, device, action_dim, episode_length, seed, action_repeat)

    def _step_launch(self, action, reset_all, out):
        launch("drq_vec_finger_step", ptr(self.phys), ptr(self.target), ptr(self.t), ptr(self.episode), ptr(self.over),
               self.N, self.A, ptr(action), self.seed, self.episode_length, self.action_repeat, int(reset_all),
               self.MODES.index(self.mode), self.target_radius, int(self.sparse), *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        launch("drq_vec_finger_render", ptr(self.phys), ptr(self.target), self.N, self.MODES.index(self.mode),
               self.target_radius, ptr(frame), device=self.device)

    def _config(self):
        return dict(super()._config(), mode=self.mode, target_radius=self.target_radius, sparse=self.sparse)


class VecMaze(_VecTask):
    """N environments of the maze on the device: the world [-1, 1]^2 is cut into size x size cells (size 3, 4, 6, 7 or 8),
    and action[:, :2] in [-1, 1] moves a point by up to 0.05 per axis and simulator step (NaN counts as 0; further columns
    are ignored), x first, then y.  A move towards a wall or the boundary stops 0.04 in front of it; no wall is crossed
    and no corner is cut.  sparse=True pays 1 for every simulator step that ends in the goal cell and 0 otherwise;
    sparse=False pays (size^2 - d) / size^2 of the geodesic distance d in cells instead, a dense shaping for debugging and
    as the comparison arm of a demo.  The rule is in include/drqv2_hip.h ("Maze") to the bit and restated by
    tests/vec_maze_oracle.py.

        env = VecMaze(num_envs=N, device="cuda", action_dim=2, episode_length=200, seed=0, action_repeat=1, size=6,
                      loops=0, layouts=0, layout_seed=0, sparse=True)

    A reset draws the start cell, the goal cell (another one) and the walls, all on the device from a hash of (seed,
    environment, episode): a spanning tree of the cells (connected by construction, size^2 - 1 open sides), one of the 8
    symmetries of the square, and with loops = 1 .. 254 every wall still closed opened with probability loops / 256
    (loops = 255 opens every wall: an empty room).
    layouts = 0 generates a fresh maze every episode; layouts = K (up to 65,535) draws one of K mazes per episode, which
    (layout_seed, index) name and all environments share -- another layout_seed is another pool, so

        train = VecMaze(N, "cuda", layouts=16, layout_seed=0)
        held_out = VecMaze(N, "cuda", layouts=16, layout_seed=1, seed=1)

    differ in the mazes and in nothing else.  Start and goal are always drawn per episode.

    The discount is 1 on every row and only the time limit (t == episode_length, in simulator steps) ends an episode, so a
    macro step's sparse reward is an exact small integer.  The frame shows the goal cell (a green inset square), the
    walls (white) and the agent (a magenta disc) over the ramp every task here draws.  geodesic() is the length in cells
    of the shortest path that is left, for an evaluation to report beside the return.  Same methods and guarantees as
    VecReach (_VecTask holds them).  The state words are "pos", float32 [N, 2]; "walls", int64 [N, 2] = the east and the
    south board, cell (r, c) bit 8 r + c, read as unsigned on the device; "cells", int32 [N, 2] = start and goal, each
    8 r + c; and t, episode, over.  The walls are state, so a checkpoint does not depend on the generator; the config of a
    state dict carries size, loops, layouts, layout_seed and sparse."""
    TASK = "maze"
    _STATE = ("pos", "walls", "cells", "t", "episode", "over")
    _STATE_SPEC = dict(_VecTask._STATE_SPEC, walls=((2,), torch.int64), cells=((2,), torch.int32))
    SIZES = (3, 4, 6, 7, 8)
    MAX_LOOPS, MAX_LAYOUTS = 255, 65535

    def __init__(self, num_envs, device, action_dim=2, episode_length=200, seed=0, action_repeat=1, size=6, loops=0,
                 layouts=0, layout_seed=0, sparse=True):
        def whole(v):
            return isinstance(v, int) and not isinstance(v, bool)
        if not whole(size) or size not in self.SIZES:
            raise ValueError(f"size must be one of {self.SIZES}, got {size!r}")
        if not whole(loops) or not 0 <= loops <= self.MAX_LOOPS:
            raise ValueError(f"loops must be an int in 0 .. {self.MAX_LOOPS}, got {loops!r}")
        if not whole(layouts) or not 0 <= layouts <= self.MAX_LAYOUTS:
            raise ValueError(f"layouts must be an int in 0 .. {self.MAX_LAYOUTS}, got {layouts!r}")
        if not whole(layout_seed):
            raise ValueError(f"layout_seed must be an int, got {layout_seed!r}")
        if not isinstance(sparse, (bool, int)) or sparse not in (0, 1):
            raise ValueError(f"sparse must be True or False, got {sparse!r}")
        self.size, self.loops, self.layouts = size, loops, layouts
        self.layout_seed, self.sparse = layout_seed & 0xFFFFFFFF, bool(sparse)
        super().__init__(num_envs, device, action_dim, episode_length, seed, action_repeat)
        self._geodesic = None       # two int32 [N] buffers used in turn, then the index of the next

    def _step_launch(self, action, reset_all, out):
        launch("drq_vec_maze_step", ptr(self.pos), ptr(self.walls), ptr(self.cells), ptr(self.t), ptr(self.episode),
               ptr(self.over), self.N, self.A, ptr(action), self.seed, self.episode_length, self.action_repeat,
               int(reset_all), self.size, self.loops, self.layouts, self.layout_seed, int(self.sparse),
               *(ptr(o) for o in out), device=self.device)

    def _render_launch(self, frame):
        launch("drq_vec_maze_render", ptr(self.pos), ptr(self.walls), ptr(self.cells), self.N, self.size, ptr(frame),
               device=self.device)

    def geodesic(self):
        """The geodesic distance in cells from the cell every agent is in to its goal cell, int32 [N] on the device: the
        flood fill of the reward, one launch (drq_vec_maze_geodesic), nothing waits.  After reset() it is the length of
        the optimal path of the episode; size^2 where walls written through load_state_dict() cut the goal off.  Two
        buffers are used in turn, like the output sets."""
        self._on_gpu()
        if self._frame is None:
            raise _lib.DrqError("geodesic(): call reset() or load_state_dict() first")
        if self._geodesic is None:
            self._geodesic = [torch.empty(self.N, dtype=torch.int32, device=self.device) for _ in range(2)] + [0]
        out = self._geodesic[self._geodesic[2]]
        self._geodesic[2] ^= 1
        launch("drq_vec_maze_geodesic", ptr(self.walls), ptr(self.cells), ptr(self.pos), self.N, self.size, ptr(out),
               device=self.device)
        return out

    def _config(self):
        return dict(super()._config(), size=self.size, loops=self.loops, layouts=self.layouts,
                    layout_seed=self.layout_seed, sparse=self.sparse)
