"""bench.py around its timed steps: a plain run is the default (--full off), and --dump-outputs writes the same files,
dtypes and values for the same agent, within the 64 MB limit (CPU: the agent's networks at the bench's shapes)."""
import types

import numpy as np
import pytest
import torch

import bench
import drqv2


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


@pytest.mark.parametrize("task", ["cheetah_run", "humanoid_run"])
def test_dump_outputs_is_repeatable_and_bounded(tmp_path, task):
    A, F, _, _ = bench.TASKS[task]
    torch.manual_seed(0)
    enc = drqv2.Encoder((9, 84, 84))
    actor = drqv2.Actor(enc.repr_dim, (A,), F, bench.H)
    critic = drqv2.Critic(enc.repr_dim, (A,), F, bench.H)
    target = drqv2.Critic(enc.repr_dim, (A,), F, bench.H)
    agent = types.SimpleNamespace(encoder=enc, actor=actor, critic=critic, critic_target=target)
    metrics = {"critic_loss": 0.25, "actor_ent": 8.5}
    for d in ("a", "b"):
        bench.dump_outputs(agent, metrics, str(tmp_path / d))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir())
    n_params = sum(len(m.state_dict()) for m in (enc, actor, critic, target))
    assert len(files) == len(metrics) + n_params
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= bench.DUMP_MAX_BYTES
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    assert float(np.load(tmp_path / "a" / "critic_loss.npy")) == 0.25
    # small tensors whole, the trunk weights (39200 x F) as a sample of their own elements
    bias = np.load(tmp_path / "a" / "critic.Q1.0.bias.npy")
    assert np.array_equal(bias, critic.Q1[0].bias.detach().numpy())
    w = np.load(tmp_path / "a" / "actor.trunk.0.weight.npy")
    assert w.size == bench.DUMP_MAX_ELEMS < actor.trunk[0].weight.numel()
    assert np.isin(w, actor.trunk[0].weight.detach().numpy().ravel()).all()
