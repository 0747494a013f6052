"""Drop-in `drqv2` module: the Hydra target `drqv2.DrQV2Agent` (cfgs/config.yaml:35 of the reference)
with the reference's constructor surface, backed by the MI355X HIP library (libdrqv2_hip.so).

Reference: /root/reference/drqv2.py.  Parity contract (tests/):
  * constructors keep names, argument order, sub-module names and state_dict keys
    (convnet.{0,2,4,6}, trunk.{0,1}, policy.{0,2,4}, Q{1,2}.{0,2,4}) and consume the global torch
    RNG exactly like the reference (same nn layers built in the same order, same init);
  * update() issues the four random draws of the reference in its order (drqv2.py:34-38 twice,
    utils.py:119 twice) and runs aug -> encoder -> critic step -> actor step -> target update in
    hand-written HIP kernels; there is no PyTorch/CPU fallback for that path;
  * metrics: the same 8 keys as python floats when use_tb, {} on gated-off steps;
  * set_behavior_cloning(alpha) (new, not in the reference): DrQ+BC, the TD3+BC actor loss fused into update();
  * dormant_ratio(obs) / perturb(alpha) (new): DrM's two primitives beside the unchanged update().
"""
import math

import numpy as np
import torch
import torch.nn as nn

import utils
from drqv2_amd import _lib, autograd, ops
from drqv2_amd.engine import StepEngine, shard_bounds
from torch.distributions.utils import _standard_normal


class RandomShiftsAug(nn.Module):
    """Random shift by up to `pad` pixels: replicate pad + bilinear resample (drqv2.py:14-45)."""

    def __init__(self, pad):
        super().__init__()
        self.pad = pad

    def draw(self, n, device, dtype=torch.float32):
        # identical call to drqv2.py:34-38 -> identical shifts under the same seed/device
        return torch.randint(0, 2 * self.pad + 1, size=(n, 1, 1, 2), device=device, dtype=dtype)

    def forward(self, x):
        n, c, h, w = x.size()
        assert h == w
        shift = self.draw(n, x.device, torch.float32)
        # differentiable in a float frame (drqv2_amd.autograd: the input gradient runs on drq_aug_bwd_f32)
        return autograd.random_shifts_aug(x.contiguous(), shift, self.pad)


class Encoder(nn.Module):
    def __init__(self, obs_shape):
        super().__init__()
        assert len(obs_shape) == 3
        self.repr_dim = 32 * 35 * 35
        layers = [nn.Conv2d(obs_shape[0], 32, 3, stride=2), nn.ReLU()]
        for _ in range(3):
            layers += [nn.Conv2d(32, 32, 3, stride=1), nn.ReLU()]
        self.convnet = nn.Sequential(*layers)
        self.apply(utils.weight_init)

    def forward(self, obs):
        """obs: uint8 or float [B,C,84,84] on the GPU -> [B, 39200] (drqv2.py:63-67), differentiable in the conv
        parameters and in a float obs (drqv2_amd.autograd.EncoderFn)."""
        if obs.dtype == torch.uint8:
            x = ops.u8_normalize(obs.contiguous())
        else:
            x = (obs.float() / 255.0 - 0.5).contiguous()
        return autograd.encoder(self, x)


def _trunk(seq, obs):
    return autograd.trunk(seq, obs.contiguous())


def _mlp3(seq, x, tanh_out=False):
    return autograd.mlp3(seq, x, tanh_out)


class Actor(nn.Module):
    def __init__(self, repr_dim, action_shape, feature_dim, hidden_dim):
        super().__init__()
        self.trunk = nn.Sequential(nn.Linear(repr_dim, feature_dim), nn.LayerNorm(feature_dim), nn.Tanh())
        self.policy = nn.Sequential(nn.Linear(feature_dim, hidden_dim), nn.ReLU(inplace=True),
                                    nn.Linear(hidden_dim, hidden_dim), nn.ReLU(inplace=True),
                                    nn.Linear(hidden_dim, action_shape[0]))
        self.apply(utils.weight_init)

    def forward(self, obs, std):
        mu = _mlp3(self.policy, _trunk(self.trunk, obs), tanh_out=True)
        return utils.TruncatedNormal(mu, torch.ones_like(mu) * std)


class Critic(nn.Module):
    def __init__(self, repr_dim, action_shape, feature_dim, hidden_dim):
        super().__init__()
        self.trunk = nn.Sequential(nn.Linear(repr_dim, feature_dim), nn.LayerNorm(feature_dim), nn.Tanh())

        def q_head():
            return nn.Sequential(nn.Linear(feature_dim + action_shape[0], hidden_dim), nn.ReLU(inplace=True),
                                 nn.Linear(hidden_dim, hidden_dim), nn.ReLU(inplace=True), nn.Linear(hidden_dim, 1))

        self.Q1 = q_head()
        self.Q2 = q_head()
        self.apply(utils.weight_init)

    def forward(self, obs, action):
        h_action = torch.cat([_trunk(self.trunk, obs), action], dim=-1).contiguous()
        return _mlp3(self.Q1, h_action), _mlp3(self.Q2, h_action)


class DrQV2Agent:
    def __init__(self, obs_shape, action_shape, device, lr, feature_dim, hidden_dim, critic_target_tau,
                 num_expl_steps, update_every_steps, stddev_schedule, stddev_clip, use_tb):
        self._init_kwargs = dict(obs_shape=tuple(obs_shape), action_shape=tuple(action_shape), device=device, lr=lr,
                                 feature_dim=feature_dim, hidden_dim=hidden_dim,
                                 critic_target_tau=critic_target_tau, num_expl_steps=num_expl_steps,
                                 update_every_steps=update_every_steps, stddev_schedule=stddev_schedule,
                                 stddev_clip=stddev_clip, use_tb=use_tb)
        self.device = device
        self.critic_target_tau = critic_target_tau
        self.update_every_steps = update_every_steps
        self.use_tb = use_tb
        self.num_expl_steps = num_expl_steps
        self.stddev_schedule = stddev_schedule
        self.stddev_clip = stddev_clip

        # models: same construction order as drqv2.py:137-145 (RNG stream parity)
        self.encoder = Encoder(obs_shape).to(device)
        self.actor = Actor(self.encoder.repr_dim, action_shape, feature_dim, hidden_dim).to(device)
        self.critic = Critic(self.encoder.repr_dim, action_shape, feature_dim, hidden_dim).to(device)
        self.critic_target = Critic(self.encoder.repr_dim, action_shape, feature_dim, hidden_dim).to(device)
        self.critic_target.load_state_dict(self.critic.state_dict())

        # arenas + fused optimisers (replace the three torch.optim.Adam of drqv2.py:148-150)
        self._engine = StepEngine(self.encoder, self.actor, self.critic, self.critic_target, obs_shape,
                                  action_shape[0], feature_dim, hidden_dim, lr, device)
        self.encoder_opt = self._engine.encoder_opt
        self.actor_opt = self._engine.actor_opt
        self.critic_opt = self._engine.critic_opt

        self.aug = RandomShiftsAug(pad=4)
        self._draw_hook = None     # tests inject the four random draws here
        # False: update() returns python floats like the reference (its .item() calls, drqv2.py:191-198,223-226).
        # True: it returns 0-d DEVICE tensors and never waits for the GPU; Logger.log() calls .item() on tensors
        # itself (logger.py:143-144), so train.py works unchanged and the wait moves to the logging cadence.
        self.metrics_on_device = False
        self.last_dormant = None           # dormant_ratio(): {layer: (dormant, units, layer mean)} of the last call
        self.last_dormant_scores = None    # ... and {layer: scores}

        self.train()
        self.critic_target.train()

    def set_compute_dtype(self, dtype):
        """"fp32" (default: the reference's arithmetic) or "bf16" (BASELINE configs[4]; new functionality): the update's
        conv2..4 and nn.Linear GEMMs run on the bf16 MFMA with fp32 accumulation and fp32 storage (DrqStep.bf16)."""
        name = {"fp32": "fp32", "f32": "fp32", "float32": "fp32", torch.float32: "fp32",
                "bf16": "bf16", "bfloat16": "bf16", torch.bfloat16: "bf16"}.get(dtype)
        if name is None:
            raise ValueError(f"compute dtype {dtype!r}: 'fp32' or 'bf16'")
        if name == "bf16" and self._engine.bc_alpha is not None:
            raise _lib.DrqError(self._engine._BC_BF16)
        self._engine.bf16 = name == "bf16"
        return self

    def set_behavior_cloning(self, alpha):
        """DrQ+BC for offline training from a fixed dataset (TD3+BC on the DrQ-v2 actor step; new functionality, the
        reference has no such loss).  alpha=None (default) is the plain update.  With alpha > 0 the critic step is
        unchanged and the actor step, on the same sample a (fourth draw, gradient straight through to mu), minimises
            -lambda * mean_i Qmin_i + mean_{i,j} (a - a_beh)^2,   lambda = alpha / mean_i |Qmin_i|  (no gradient),
        a_beh being the batch's `action`; the arithmetic runs in the BC forms of the actor-step kernels
        (include/drqv2_hip.h), launch for launch.  Metrics gain "actor_bc_loss" and "actor_bc_lambda"; "actor_loss" is
        the total.  Single GPU only."""
        if alpha is not None:
            try:
                ok = not isinstance(alpha, bool) and math.isfinite(float(alpha)) and float(alpha) > 0.0
                with np.errstate(over="ignore"):
                    ok = ok and 0.0 < float(np.float32(alpha)) < float("inf")      # the kernels take it as fp32
            except (TypeError, ValueError, OverflowError):
                ok = False
            if not ok:
                raise ValueError(f"behaviour-cloning alpha {alpha!r}: None or a finite float > 0")
            alpha = float(alpha)
        self._engine.set_behavior_cloning(alpha)
        return self

    def _bc_metrics(self, metrics, q_sum, sq_sum, abs_sum, inv):
        """actor_loss (the total), actor_bc_loss, actor_bc_lambda from the sums the BC loss kernel leaves: q_sum = sum -Qmin
        (slot 5), sq_sum = sum (a - a_beh)^2 (slot 9), abs_sum = sum |Qmin| (slot 10); floats or 0-d tensors."""
        lam = self._engine.bc_alpha / (abs_sum * inv)
        bc = sq_sum * (inv / self._engine.A)
        metrics["actor_loss"] = lam * (q_sum * inv) + bc
        metrics["actor_bc_loss"] = bc
        metrics["actor_bc_lambda"] = lam

    def train(self, training=True):
        self.training = training
        self.encoder.train(training)
        self.actor.train(training)
        self.critic.train(training)

    # ---- drqv2.py:164-175 ----------------------------------------------------------------------
    def act(self, obs, step, eval_mode):
        obs = torch.as_tensor(obs, device=self.device)
        mu = self._engine.act_forward(obs.unsqueeze(0).contiguous())
        stddev = utils.schedule(self.stddev_schedule, step)
        dist = utils.TruncatedNormal(mu, torch.ones_like(mu) * stddev)
        if eval_mode:
            action = dist.mean
        else:
            action = dist.sample(clip=None)
            if step < self.num_expl_steps:
                action.uniform_(-1.0, 1.0)
        return action.cpu().numpy()[0]

    def act_batch(self, obs, step, eval_mode):
        """act() for n observations at once (new: vectorised environments, parallel evaluation episodes, frames that
        already live on the GPU): the body of drqv2.py:164-175 without unsqueeze(0) / [0], on the inference launches of
        csrc/act.hip (drq_act_batch).
        obs: uint8 [n, C, 84, 84] -- numpy array, host tensor, or tensor on the agent's device.
        Returns float32 [n, A]: a tensor on the agent's device if obs was one (nothing waits for the GPU), otherwise a
        numpy array.
        The generator is consumed as the reference's body would on a batch: when not eval_mode ONE
        _standard_normal((n, A)) draw (TruncatedNormal.sample), then, while step < num_expl_steps, uniform_(-1, 1) over
        the [n, A] result; for n = 1 exactly what act() consumes.  Up to StepEngine.ACT_FUSED_MAX_ROWS frames the call
        does not touch the step workspace and may sit between encode() and update_critic(); larger batches go through
        act()'s kernels in chunks and must not (StepEngine.act_batch_forward)."""
        if str(self.device).startswith("cpu"):
            raise _lib.DrqError("DrQV2Agent.update/act need the GPU: the HIP path has no CPU fallback")
        on_device = isinstance(obs, torch.Tensor) and obs.is_cuda
        if not on_device:
            obs = torch.as_tensor(obs).to(self.device)
        if obs.dim() != 4:
            raise _lib.DrqError(f"act_batch(): frames of shape (n, C, 84, 84) required, got {tuple(obs.shape)}")
        eng = self._engine
        if eval_mode:
            action = eng.act_batch_forward(obs.contiguous())
        else:
            stddev = utils.schedule(self.stddev_schedule, step)
            noise = _standard_normal((obs.shape[0], eng.A), dtype=torch.float32, device=eng.device)   # utils.py:119
            action = eng.act_batch_forward(obs.contiguous(), noise, stddev)
            if step < self.num_expl_steps:
                action.uniform_(-1.0, 1.0)
        return action if on_device else action.cpu().numpy()

    # ---- DrM building blocks (new, not in the reference): dormant ratio and weight perturbation ----
    @staticmethod
    def _net_names(nets, allowed, what):
        if isinstance(nets, str):
            nets = (nets,)
        try:
            nets = tuple(nets)
        except TypeError:
            nets = (nets,)
        if not nets or len(set(nets)) != len(nets) or any(not isinstance(n, str) or n not in allowed for n in nets):
            raise ValueError(f"{what}: nets {nets!r} must be distinct names out of {allowed}")
        return tuple(n for n in allowed if n in nets)              # the order of `allowed`, whatever order was given

    @staticmethod
    def _unit_float(v, lo, hi, what):
        """a real number in [lo, hi] that is one as an fp32 too (the kernels take it as such); no bools, no NaN"""
        try:
            ok = not isinstance(v, bool) and lo <= float(v) <= hi and lo <= float(np.float32(v)) <= hi
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(what)
        return float(v)

    def dormant_ratio(self, obs, action=None, tau=0.025, nets=("actor",)):
        """The dormant ratio (Sokar et al. 2023; the quantity DrM, Xu et al. 2024, steers exploration and perturbation by)
        of the named networks on a batch, as a 0-d float32 DEVICE tensor in [0, 1]; nothing waits for the GPU.
        The contract:
          * obs: uint8 [n >= 1, 9, 84, 84] on the agent's device; action (needed by "critic"): float32 [n, A] there.
          * scored layers, each by its POST-ACTIVATION output: "actor" -- the trunk output (F units, after LayerNorm and
            tanh) and the two hidden ReLU layers of the policy (H units each); "critic" -- its trunk output and the two
            hidden layers of both Q heads (F + 4H units).  (DrM's public code hooks the nn.Linear outputs instead, so its
            numbers are not these.)
          * score_j = mean over the batch of |output_j|; unit j of a layer is dormant when score_j <= tau * (mean of the
            layer's scores), and every unit of a layer whose mean is 0 is.  The ratio is dormant units over units, summed
            over the scored layers.
        The forward is the modules' fp32 forward (also when the compute dtype of update() is bf16) without augmentation,
        in buffers of its own: n is not tied to the update's batch and the step workspace is not touched.  No gradient,
        no optimiser state and no random numbers are involved (the generators do not move); a deferred optimiser step is
        completed first, as in act().  `last_dormant` then holds {layer: (dormant, units, layer mean)} and
        `last_dormant_scores` {layer: scores}, device tensors; layers are named "actor.trunk", "actor.policy.0",
        "actor.policy.2", "critic.trunk", "critic.Q1.0", ... (the index of the nn.Linear whose activation is scored)."""
        tau = self._unit_float(tau, 0.0, 3.0e38, f"dormant_ratio(): tau {tau!r} must be a finite float >= 0")
        nets = self._net_names(nets, ("actor", "critic"), "dormant_ratio()")
        if "critic" in nets and action is None:
            raise ValueError("dormant_ratio(): the critic's layers need an action batch")
        if str(self.device).startswith("cpu"):
            raise _lib.DrqError("DrQV2Agent.update/act need the GPU: the HIP path has no CPU fallback")
        ratio, self.last_dormant, self.last_dormant_scores = self._engine.dormant_ratio(obs, action, tau, nets)
        return ratio

    def perturb(self, alpha, nets=("encoder", "actor", "critic"), generator=None):
        """DrM's perturbation: p <- alpha p + (1 - alpha) p0 for every parameter of the named networks, p0 a fresh
        initialisation -- throw-away modules of the same constructors (the reference's weight_init), built on the CPU in
        the order encoder, actor, critic from `generator` (a CPU torch.Generator, which is advanced) or else from the
        global torch generator -- copied to the device once and applied by one launch per parameter segment.
        "critic" pulls critic_target toward the SAME p0, so the target keeps its relation to the critic.  The Adam
        moments and step counts are left as they are.  alpha is a float in [0, 1]: 1 changes nothing, launches nothing
        and draws nothing; 0 is a re-initialisation.  A deferred optimiser step is completed first.  Single GPU only.
        Stateless: a checkpoint has nothing to save for it."""
        alpha = self._unit_float(alpha, 0.0, 1.0, f"perturb(): alpha {alpha!r} must be a float in [0, 1]")
        nets = self._net_names(nets, ("encoder", "actor", "critic"), "perturb()")
        if generator is not None and (not isinstance(generator, torch.Generator) or generator.device.type != "cpu"):
            raise ValueError("perturb(): generator must be a CPU torch.Generator")
        if str(self.device).startswith("cpu"):
            raise _lib.DrqError("DrQV2Agent.update/act need the GPU: the HIP path has no CPU fallback")
        if self._engine.pg is not None:
            raise _lib.DrqError(self._engine._PERTURB_DP)
        if alpha == 1.0:
            return self
        kw = self._init_kwargs
        dims = (self.encoder.repr_dim, kw["action_shape"], kw["feature_dim"], kw["hidden_dim"])
        make = {"encoder": lambda: Encoder(kw["obs_shape"]), "actor": lambda: Actor(*dims), "critic": lambda: Critic(*dims)}
        if generator is None:
            fresh = {n: make[n]() for n in nets}
        else:
            with torch.random.fork_rng(devices=[]):          # the constructors draw from the global generator
                torch.random.set_rng_state(generator.get_state())
                fresh = {n: make[n]() for n in nets}
                generator.set_state(torch.random.get_rng_state())
        self._engine.perturb(alpha, {"enc" if n == "encoder" else n: m for n, m in fresh.items()})
        return self

    # ---- data parallel (new: one process per GPU, RCCL all-reduce of the flat gradient arenas) ---
    def enable_data_parallel(self, process_group=None, batch_is_global=True, global_metrics=False,
                             exchange="allreduce"):
        """batch_is_global: every rank's replay_iter yields the same global batch and this rank trains
        on its contiguous slice; otherwise the iterator already yields this rank's shard.
        global_metrics: the returned metrics are means over the GLOBAL batch (one more 32-byte all-reduce per
        update); by default they are the means over this rank's shard (the gradients are always global).
        exchange: "allreduce" | "direct" | "zero1" | "auto" -- drqv2_amd.engine.GradExchange ("zero1": Adam sharded over the
        ranks, each steps 1/world of every segment and the stepped parameters are all-gathered)."""
        self._engine.enable_data_parallel(process_group, global_metrics, exchange)
        self._batch_is_global = batch_is_global

    def _draws(self, n_global, A):
        if self._draw_hook is not None:
            return self._draw_hook(n_global, A)
        dev = self.device
        fused = self._engine.rng_draws(n_global, A, 2 * self.aug.pad + 1)           # the same four draws, one launch
        if fused is not None:
            return fused
        sh_o = self.aug.draw(n_global, dev)                                        # RNG draw 1 (drqv2.py:241)
        sh_n = self.aug.draw(n_global, dev)                                        # RNG draw 2 (:242)
        n_c = _standard_normal((n_global, A), dtype=torch.float32, device=dev)     # draw 3 (:183)
        n_a = _standard_normal((n_global, A), dtype=torch.float32, device=dev)     # draw 4 (:211)
        return sh_o, sh_n, n_c, n_a

    # ---- drqv2.py:230-262 ----------------------------------------------------------------------
    def update(self, replay_iter, step):
        metrics = dict()
        if step % self.update_every_steps != 0:
            return metrics

        batch = next(replay_iter)
        frames = getattr(batch, "frames", None)      # drqv2_amd.replay.IndexedBatch: obs / next_obs are indices into it
        # prioritized replay (drqv2_amd.replay.PrioritizedBatch, or any batch type of the caller's with this attribute):
        # float32 [B] on the device, the critic loss becomes mean_i w_i (Q - y)_i^2 per head (StepEngine.update)
        weights = getattr(batch, "weights", None)
        wkw = {} if weights is None else {"loss_weights": weights}
        # drqv2_amd.replay.FrameBatch: `frames` is a ring of single frames, the indices name the newest frame of each
        # stack and the ring's flags tell the fused aug+conv1 launch where the other two are (StepEngine.update)
        if getattr(batch, "ring", None) is not None:
            wkw["ring"] = batch.ring
        obs, action, reward, discount, next_obs = utils.to_torch(batch, self.device)
        eng = self._engine
        A = eng.A
        world, rank = eng.world, eng.rank
        big = getattr(self, "_batch_is_global", True)
        lo, hi, n_global = shard_bounds(obs.shape[0], world, rank, big)
        if world > 1 and big:
            obs_l, action_l, reward_l, discount_l, next_l = (t[lo:hi] for t in (obs, action, reward, discount,
                                                                                 next_obs))
        else:
            obs_l, action_l, reward_l, discount_l, next_l = obs, action, reward, discount, next_obs
        # every rank draws for the GLOBAL batch and keeps its slice: same numbers as the 1-GPU run
        sh_o, sh_n, n_c, n_a = (t.reshape(n_global, -1)[lo:hi].contiguous() for t in self._draws(n_global, A))

        stddev = utils.schedule(self.stddev_schedule, step)
        f32 = lambda t: t.to(torch.float32).contiguous()
        if frames is not None:
            sums = eng.update(frames, f32(action_l), f32(reward_l).view(-1), f32(discount_l).view(-1), frames, f32(sh_o),
                              f32(sh_n), f32(n_c), f32(n_a), stddev, self.stddev_clip, self.critic_target_tau,
                              B_global=n_global, obs_index=obs_l.contiguous(), next_obs_index=next_l.contiguous(), **wkw)
        else:
            sums = eng.update(obs_l.contiguous(), f32(action_l), f32(reward_l).view(-1), f32(discount_l).view(-1),
                              next_l.contiguous(), f32(sh_o), f32(sh_n), f32(n_c), f32(n_a), stddev, self.stddev_clip,
                              self.critic_target_tau, B_global=n_global, **wkw)

        # the per-sample |TD error| of this update goes back into the store's priorities, in stream order (no host wait)
        # and before the iterator below places new episodes and draws again
        renew = getattr(batch, "update_priorities", None) if weights is not None else None
        if renew is not None:
            renew(eng.last_td_abs)
        # the update is queued: the next batch's host work goes here, beside the GPU (drqv2_amd.replay.BatchIterator)
        ahead = getattr(replay_iter, "prefetch", None)
        if ahead is not None:
            ahead()
        if self.use_tb and self.metrics_on_device:
            inv = 1.0 / (n_global if (eng.pg is None or eng.global_metrics) else (hi - lo))
            if eng._side_busy:           # data parallel with global metrics: the sums exchange runs on a side stream
                torch.cuda.current_stream(eng.device).wait_stream(eng._side)
            vals = sums[:7] * inv        # a fresh tensor: the sums buffer is overwritten by the next update
            for i, k in enumerate(("batch_reward", "critic_target_q", "critic_q1", "critic_q2", "critic_loss",
                                   "actor_loss", "actor_logprob")):
                metrics[k] = vals[i]
            metrics["actor_ent"] = torch.tensor(A * (0.5 + 0.5 * math.log(2 * math.pi) + math.log(stddev)),
                                                dtype=torch.float32)
            if eng.bc_alpha is not None:
                bc = eng.bc_sums.clone()     # like vals: the buffer is overwritten by the next update
                self._bc_metrics(metrics, sums[5], bc[0], bc[1], inv)
        elif self.use_tb:
            s = eng.read_sums()          # the single device->host wait of the update
            # data parallel without global_metrics: the sums cover this rank's rows only
            inv = 1.0 / (n_global if (eng.pg is None or eng.global_metrics) else (hi - lo))
            metrics["batch_reward"] = s[0] * inv
            metrics["critic_target_q"] = s[1] * inv
            metrics["critic_q1"] = s[2] * inv
            metrics["critic_q2"] = s[3] * inv
            metrics["critic_loss"] = s[4] * inv
            metrics["actor_loss"] = s[5] * inv
            metrics["actor_logprob"] = s[6] * inv
            metrics["actor_ent"] = A * (0.5 + 0.5 * math.log(2 * math.pi) + math.log(stddev))
            if eng.bc_alpha is not None:
                self._bc_metrics(metrics, s[5], *eng.read_bc_sums(), inv)
        return metrics

    # ---- the update in the reference's pieces (drqv2.py:177-228, :241-246) -----------------------------------------
    def encode(self, obs, next_obs, step):
        """aug + encoder of both views as update() does (drqv2.py:241-246), for callers that issue update_critic /
        update_actor themselves: obs / next_obs uint8 [B,C,84,84]; returns the features (obs, next_obs) [B, 39200], views
        of the step workspace.  Consumes the two shift draws of the reference.  The encoder's backward inside
        update_critic uses the activations THIS call saved (the autograd graph of the reference's `self.encoder(obs)`)."""
        obs, next_obs = (torch.as_tensor(t, device=self.device).contiguous() for t in (obs, next_obs))
        n = obs.shape[0]
        sh_o, sh_n = self.aug.draw(n, self.device), self.aug.draw(n, self.device)      # RNG draws 1, 2
        stddev = utils.schedule(self.stddev_schedule, step)
        return self._engine.begin_manual(obs, next_obs, sh_o.reshape(n, 2).contiguous(), sh_n.reshape(n, 2).contiguous(),
                                         stddev, self.stddev_clip, self.critic_target_tau)

    def update_critic(self, obs, action, reward, discount, next_obs, step):
        """drqv2.py:177-204.  obs / next_obs: the features encode() returned for this batch.  Issues the critic loss, its
        backward through the encoder, critic_opt.step() and encoder_opt.step(); consumes the reference's third draw
        (utils.py:119).  `step` must be the step encode() was called with (the stddev schedule is evaluated there).
        Always the unweighted loss: the importance weights of prioritized replay go through update() only."""
        metrics = dict()
        f32 = lambda t: torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
        n = obs.shape[0]
        n_c = _standard_normal((n, self._engine.A), dtype=torch.float32, device=self.device)   # draw 3 (:183)
        sums = self._engine.manual_critic(obs, f32(action), f32(reward).view(-1), f32(discount).view(-1), next_obs, n_c)
        if self.use_tb:
            s = sums.tolist()
            inv = 1.0 / n
            metrics["critic_target_q"] = s[1] * inv
            metrics["critic_q1"] = s[2] * inv
            metrics["critic_q2"] = s[3] * inv
            metrics["critic_loss"] = s[4] * inv
        return metrics

    def update_actor(self, obs, step):
        """drqv2.py:206-228, after update_critic of the same batch.  Consumes the reference's fourth draw."""
        metrics = dict()
        m = getattr(self._engine, "_manual", None)
        if m is None:
            raise _lib.DrqError("update_actor(): call update_critic() for this batch first")
        n, A = m["B"], self._engine.A
        n_a = _standard_normal((n, A), dtype=torch.float32, device=self.device)               # draw 4 (:211)
        stddev = utils.schedule(self.stddev_schedule, step)
        sums = self._engine.manual_actor(n_a)
        if self.use_tb:
            s = sums.tolist()
            inv = 1.0 / n
            metrics["actor_loss"] = s[5] * inv
            metrics["actor_logprob"] = s[6] * inv
            metrics["actor_ent"] = A * (0.5 + 0.5 * math.log(2 * math.pi) + math.log(stddev))
            if self._engine.bc_alpha is not None:
                self._bc_metrics(metrics, s[5], *self._engine.bc_sums.tolist(), inv)
        return metrics

    # ---- snapshots: train.py:192-204 pickles the whole agent --------------------------------
    def flush(self):
        """Data parallel only: finish the Adam(actor) step the last update() left overlapped with its gradient
        all-reduce.  update(), act() and snapshots do this themselves; call it before reading actor weights
        directly."""
        self._engine.flush()

    # ---- weights-only interchange with the reference's classes -----------------------------
    def export_reference_state(self):
        """The agent as plain tensors in the formats the REFERENCE's objects load with their own methods:
        `state_dict()`s of the four nn.Modules (same keys: drqv2.py:48-121) and `torch.optim.Adam.state_dict()`s of the
        three optimisers (drqv2.py:148-150: per-parameter `step`, `exp_avg`, `exp_avg_sq`, one param group).
        No code is pickled: `torch.save(agent.export_reference_state(), f)` loads with `weights_only=True`, and a
        reference agent takes it with `agent.encoder.load_state_dict(s["encoder"])` ...
        `agent.encoder_opt.load_state_dict(s["encoder_opt"])`."""
        self._engine.flush()
        self._engine.gather_optimizer_state()
        cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
        out = {"format": "drqv2-reference-state-v1",
               "encoder": cpu(self.encoder.state_dict()), "actor": cpu(self.actor.state_dict()),
               "critic": cpu(self.critic.state_dict()), "critic_target": cpu(self.critic_target.state_dict())}
        eng = self._engine
        for net, opt_name, mod in (("enc", "encoder_opt", self.encoder), ("actor", "actor_opt", self.actor),
                                   ("critic", "critic_opt", self.critic)):
            opt = getattr(self, opt_name)
            state = {}
            plist = list(mod.parameters())
            if opt.t > 0:
                for i, (p, off) in enumerate(zip(plist, eng.layout[net])):
                    n = p.numel()
                    state[i] = {"step": torch.tensor(float(opt.t)),
                                "exp_avg": eng.adam_m[off:off + n].view(p.shape).detach().cpu().clone(),
                                "exp_avg_sq": eng.adam_v[off:off + n].view(p.shape).detach().cpu().clone()}
            group = dict(lr=opt.lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                         foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                         params=list(range(len(plist))))
            out[opt_name] = {"state": state, "param_groups": [group]}
        return out

    def import_reference_state(self, st):
        """The reverse: weights, target and Adam state from `export_reference_state()`-shaped data, e.g. what a
        reference agent produces with {name: module.state_dict()} and {name: optimiser.state_dict()}."""
        # data parallel: the deferred Adam(encoder/actor) of the last update must land BEFORE the imported weights do
        self._engine.flush()
        for n in ("encoder", "actor", "critic", "critic_target"):
            getattr(self, n).load_state_dict(st[n])
        eng = self._engine
        for net, opt_name, mod in (("enc", "encoder_opt", self.encoder), ("actor", "actor_opt", self.actor),
                                   ("critic", "critic_opt", self.critic)):
            mine = getattr(self, opt_name)
            ref = st[opt_name]["state"]
            t = 0
            for i, (p, off) in enumerate(zip(mod.parameters(), eng.layout[net])):
                ent = ref.get(i, ref.get(str(i)))
                if ent is None:
                    # no state for this parameter in the reference optimiser (it has not stepped): fresh moments, not
                    # whatever this agent had accumulated (bias correction restarts at t = 0)
                    eng.adam_m[off:off + p.numel()].zero_()
                    eng.adam_v[off:off + p.numel()].zero_()
                    continue
                m, v = ent["exp_avg"], ent["exp_avg_sq"]
                eng.adam_m[off:off + m.numel()].copy_(m.reshape(-1))
                eng.adam_v[off:off + v.numel()].copy_(v.reshape(-1))
                t = max(t, int(ent["step"]))
            mine.t = t
            mine.param_groups[0]["lr"] = st[opt_name]["param_groups"][0]["lr"]

    def __getstate__(self):
        self._engine.flush()
        self._engine.gather_optimizer_state()       # sharded optimiser: every rank's snapshot holds complete moments
        cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
        return {"init": self._init_kwargs, "training": self.training,
                "encoder": cpu(self.encoder.state_dict()), "actor": cpu(self.actor.state_dict()),
                "critic": cpu(self.critic.state_dict()), "critic_target": cpu(self.critic_target.state_dict()),
                "opt": {n: getattr(self, n).export_state() for n in ("encoder_opt", "actor_opt", "critic_opt")},
                "bc_alpha": self._engine.bc_alpha, "compute_dtype": "bf16" if self._engine.bf16 else "fp32"}

    def _load_reference_state(self, st):
        """`st` is the __dict__ of an agent pickled by the REFERENCE's class (train.py:192-198 pickles the object and
        the reference defines no __getstate__): nn.Modules, torch.optim.Adam objects, scalar attributes.  With this
        module on the path pickle resolves `drqv2.DrQV2Agent` to this class and hands that dict over here; the agent
        is rebuilt on the arenas, weights and Adam moments are copied in."""
        cpu = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
        sds = {n: cpu(st[n]) for n in ("encoder", "actor", "critic", "critic_target")}
        a = sds["actor"]
        dev = st.get("device", "cuda")
        if str(dev).startswith("cuda") and not torch.cuda.is_available():
            dev = "cpu"
        kw = dict(obs_shape=(sds["encoder"]["convnet.0.weight"].shape[1], 84, 84),
                  action_shape=(a["policy.4.weight"].shape[0],), device=dev,
                  lr=st["actor_opt"].param_groups[0]["lr"], feature_dim=a["trunk.0.weight"].shape[0],
                  hidden_dim=a["policy.0.weight"].shape[0], critic_target_tau=st["critic_target_tau"],
                  num_expl_steps=st["num_expl_steps"], update_every_steps=st["update_every_steps"],
                  stddev_schedule=st["stddev_schedule"], stddev_clip=st["stddev_clip"], use_tb=st["use_tb"])
        with torch.random.fork_rng(devices=[]):
            self.__init__(**kw)
        for n, sd in sds.items():
            getattr(self, n).load_state_dict(sd)
        eng = self._engine
        for net, opt_name in (("enc", "encoder_opt"), ("actor", "actor_opt"), ("critic", "critic_opt")):
            ref = st[opt_name].state_dict()["state"]          # param index -> {step, exp_avg, exp_avg_sq}
            mine = getattr(self, opt_name)
            t = 0
            for i, off in enumerate(eng.layout[net]):
                if i not in ref:
                    continue
                m, v = ref[i]["exp_avg"], ref[i]["exp_avg_sq"]
                eng.adam_m[off:off + m.numel()].copy_(m.reshape(-1))
                eng.adam_v[off:off + v.numel()].copy_(v.reshape(-1))
                t = max(t, int(ref[i]["step"]))
            mine.t = t
        self.train(bool(st.get("training", True)))

    def __setstate__(self, st):
        if "init" not in st:
            return self._load_reference_state(st)
        kw = dict(st["init"])
        if str(kw["device"]).startswith("cuda") and not torch.cuda.is_available():
            kw["device"] = "cpu"
        with torch.random.fork_rng(devices=[]):      # building the nets must not move the global RNG
            self.__init__(**kw)
        self._restore(st)

    def _restore(self, st):
        """what __setstate__ does once the agent is built: weights, target, Adam moments and step counts, the DrQ+BC and
        compute-dtype settings, the training flag -- copied into the arenas of THIS agent.  drqv2_amd.checkpoint.load()
        calls it on a live agent whose constructor arguments it has compared with st["init"]."""
        self._engine.flush()        # data parallel: a deferred Adam step must land before the restored weights do
        self.encoder.load_state_dict(st["encoder"])
        self.actor.load_state_dict(st["actor"])
        self.critic.load_state_dict(st["critic"])
        self.critic_target.load_state_dict(st["critic_target"])
        for n, s in st["opt"].items():
            getattr(self, n).import_state(s)
        dtype = st.get("compute_dtype")                    # absent in snapshots written before it was saved: as it is
        if dtype == "fp32":
            self.set_compute_dtype("fp32")
        self.set_behavior_cloning(st.get("bc_alpha"))      # absent in snapshots written before DrQ+BC: off
        if dtype == "bf16":
            self.set_compute_dtype("bf16")
        self.train(st["training"])
