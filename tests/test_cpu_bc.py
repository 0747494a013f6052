"""DrQ+BC (DrQV2Agent.set_behavior_cloning): everything that needs no GPU.  The public surface (setter, snapshots, the
refusals), and the closed-form gradients the kernels implement against autograd of the fp64 restatement
(tests/bc_oracle.py), which pins the formulas before a GPU is involved."""
import math
import multiprocessing as mp
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

from drqv2_amd import _lib, synth
from tests import bc_oracle


@pytest.fixture(autouse=True)
def feature_present():
    """every test of this file is about DrQ+BC: without the setter none of them has a subject"""
    import drqv2
    assert callable(getattr(drqv2.DrQV2Agent, "set_behavior_cloning", None)), "DrQV2Agent.set_behavior_cloning is missing"


def agent(A=3, use_tb=False):
    import drqv2
    return drqv2.DrQV2Agent((9, 84, 84), (A,), "cpu", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, use_tb)


def test_setter_validates_and_defaults_to_off():
    ag = agent()
    assert ag._engine.bc_alpha is None
    assert ag.set_behavior_cloning(2.5) is ag and ag._engine.bc_alpha == 2.5
    assert ag.set_behavior_cloning(1) is ag and ag._engine.bc_alpha == 1.0 and isinstance(ag._engine.bc_alpha, float)
    assert ag.set_behavior_cloning(np.float32(0.5)) is ag and ag._engine.bc_alpha == 0.5
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "2.5x", [2.5], True, 1e-60, 1e39):
        with pytest.raises(ValueError):
            ag.set_behavior_cloning(bad)
        assert ag._engine.bc_alpha == 0.5                      # a refused value changes nothing
    assert ag.set_behavior_cloning(None) is ag and ag._engine.bc_alpha is None


def test_signature_and_pinned_interface_untouched():
    import inspect
    import json
    import drqv2
    assert list(inspect.signature(drqv2.DrQV2Agent.set_behavior_cloning).parameters) == ["self", "alpha"]
    with open(os.path.join(os.path.dirname(__file__), "golden", "interface.json")) as f:
        iface = json.load(f)
    assert "set_behavior_cloning" not in json.dumps(iface)     # not a constructor argument, nothing pinned moved
    assert "alpha" not in inspect.signature(drqv2.DrQV2Agent.__init__).parameters
    for name in ("drq_actor_loss_bc", "drq_qout_bwd_actor_bc", "drq_actor_dmu_bc", "drq_policy_out_bwd_bc",
                 "drq_update_phase_bc"):
        assert name in _lib.PROTOTYPES


def test_snapshot_round_trip_and_old_format():
    ag = agent().set_behavior_cloning(2.5)
    back = pickle.loads(pickle.dumps(ag))
    assert back._engine.bc_alpha == 2.5
    assert torch.equal(back._engine.params, ag._engine.params)
    st = ag.__getstate__()
    assert st["bc_alpha"] == 2.5
    del st["bc_alpha"]                                         # a snapshot written before DrQ+BC existed
    import drqv2
    old = object.__new__(drqv2.DrQV2Agent)
    old.__setstate__(st)
    assert old._engine.bc_alpha is None
    assert pickle.loads(pickle.dumps(agent()))._engine.bc_alpha is None
    assert "bc_alpha" not in ag.export_reference_state()       # the reference's objects know nothing of it


def test_bf16_combination_is_refused_in_either_order():
    ag = agent().set_behavior_cloning(2.5)
    with pytest.raises(_lib.DrqError, match="bf16"):
        ag.set_compute_dtype("bf16")
    assert ag._engine.bf16 is False and ag.set_compute_dtype("fp32") is ag
    ag = agent().set_compute_dtype("bf16")
    with pytest.raises(_lib.DrqError, match="bf16"):
        ag.set_behavior_cloning(2.5)
    assert ag._engine.bc_alpha is None
    assert ag.set_behavior_cloning(None) is ag                 # turning it off is always allowed


def test_update_phase_bc_argument_errors_come_before_any_launch():
    lib = _lib.load()
    d = _lib.DrqStep()
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.drq_update_phase_bc(d, -1, alpha) == -1
    assert lib.drq_update_phase_bc(None, -1, 2.5) == -1
    d.B, d.global_B = 8, 16                                    # data parallel: refused by the library too
    assert lib.drq_update_phase_bc(d, -1, 2.5) == -1
    assert lib.drq_actor_loss_bc(None, None, None, 6, None, 6, None, 0.2, 2.5, None, None, None, 8, 6, 0.125, None) == -1
    assert lib.drq_actor_dmu_bc(None, None, 6, 0, None, None, 6, None, 6, 0.1, None, 8, 6, None) == -1
    assert lib.drq_policy_out_bwd_bc(None, None, 6, 0, None, None, 6, None, 6, 0.1, None, None, None, None, None, 8, 64, 6,
                                     None, 0, None) == -1
    assert lib.drq_qout_bwd_actor_bc(None, None, None, 6, None, 6, None, 0.2, 2.5, 6, 0.125, None, None, None, None, 8, 64,
                                     None) == -1


def _dp_worker(path, order, ret):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=0, world_size=1)
    try:
        ag = agent()
        try:
            if order == "bc_first":
                ag.set_behavior_cloning(2.5)
                ag.enable_data_parallel()
            else:
                ag.enable_data_parallel()
                ag.set_behavior_cloning(2.5)
            ret["raised"] = None
        except _lib.DrqError as e:
            ret["raised"] = str(e)
        ret["bc_alpha"] = ag._engine.bc_alpha
        ret["pg"] = ag._engine.pg is not None
        if order != "bc_first":
            ag.set_behavior_cloning(None)                      # off stays legal with data parallelism on
            ret["off_ok"] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("order", ["bc_first", "dp_first"])
def test_data_parallel_refusal_on_a_group_of_one(order):
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as tmp, ctx.Manager() as man:
        ret = man.dict()
        p = ctx.Process(target=_dp_worker, args=(os.path.join(tmp, "store"), order, ret))
        p.start()
        p.join(180)
        assert p.exitcode == 0
        ret = dict(ret)
    assert ret["raised"] is not None and "data parallel" in ret["raised"] and "exchange" in ret["raised"], ret
    if order == "bc_first":
        assert ret["bc_alpha"] == 2.5 and ret["pg"] is False   # the refused call changed nothing
    else:
        assert ret["bc_alpha"] is None and ret["pg"] is True and ret["off_ok"]


def _problem(A, B=8, F=20, H=64, seed=0, dtype=torch.float64):
    _, actor, critic = synth.make_weights(9, A, F, H, seed)
    cv = lambda d: {k: v.to(dtype) for k, v in d.items()}
    g = torch.Generator().manual_seed(100 + A)
    feat = torch.randn(B, 39200, generator=g, dtype=dtype) * 0.05
    a_beh = torch.rand(B, A, generator=g, dtype=dtype) * 2 - 1
    noise = torch.randn(B, A, generator=g, dtype=dtype)
    return cv(actor), cv(critic), feat, a_beh, noise


def nerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("alpha", [2.5, 0.4])
@pytest.mark.parametrize("A", [1, 3, 6, 21])
def test_closed_form_gradients_equal_autograd_in_fp64(A, alpha):
    """dq = -lambda / B on the head that holds the minimum and dmu = da_1 + da_2 + 2 (a - a_beh) / (B A), the formulas
    the kernels implement, against autograd of the restatement: 1e-12 normwise in fp64."""
    actor, critic, feat, a_beh, noise = _problem(A)
    r = bc_oracle.bc_actor_step(actor, critic, feat, a_beh, noise, 0.2, 0.3, alpha)
    c = bc_oracle.closed_form(critic, feat, r["a"], a_beh, r["q1"], r["q2"], alpha)
    assert float(c["lam"]) == pytest.approx(float(r["lam"]), rel=1e-14)
    assert float(r["loss"]) == pytest.approx(float(-r["lam"] * r["qmin"].mean() + r["bc"]), rel=1e-14)
    for k in ("dq1", "dq2", "dmu"):
        e = nerr(c[k], r[k])
        print(f"A={A} alpha={alpha} {k}: closed form vs autograd {e:.3e}")
        assert e <= 1e-12, (k, e)
    # each row's gradient went to exactly one head, and the BC term is not negligible in dmu (the test would otherwise
    # not see a wrong factor on it)
    assert bool(((c["dq1"] != 0) ^ (c["dq2"] != 0)).all())
    pull = 2.0 * (r["a"] - a_beh) / (a_beh.numel())
    assert float(pull.norm() / c["dmu"].norm()) > 1e-3
    # dpre = dmu (1 - mu^2): the gradient autograd leaves at the last layer's bias is its column sum
    dpre = c["dmu"] * (1 - r["mu"] ** 2)
    assert nerr(dpre.sum(0), r["g_actor"]["policy.4.bias"]) <= 1e-12


def test_tie_splits_the_gradient_between_the_heads():
    q1 = torch.tensor([[1.0], [2.0], [-3.0]], dtype=torch.float64, requires_grad=True)
    q2 = torch.tensor([[1.0], [1.5], [-2.0]], dtype=torch.float64, requires_grad=True)
    qmin = torch.minimum(q1, q2)
    lam = (2.5 / qmin.abs().mean()).detach()
    (-lam * qmin.mean()).backward()
    g = -float(lam) / 3
    assert q1.grad.view(-1).tolist() == pytest.approx([0.5 * g, 0.0, g], rel=1e-15)
    assert q2.grad.view(-1).tolist() == pytest.approx([0.5 * g, g, 0.0], rel=1e-15)


def test_metrics_from_the_sums():
    """the host side of the metrics: actor_loss / actor_bc_loss / actor_bc_lambda from the three sums the loss kernel
    leaves, floats and 0-d tensors alike"""
    ag = agent(A=3).set_behavior_cloning(0.4)
    B, A = 8, 3
    g = torch.Generator().manual_seed(5)
    qmin = torch.randn(B, generator=g, dtype=torch.float64) + 0.3
    d = torch.randn(B, A, generator=g, dtype=torch.float64)
    lam = 0.4 / float(qmin.abs().mean())
    want = {"actor_loss": -lam * float(qmin.mean()) + float((d * d).mean()), "actor_bc_loss": float((d * d).mean()),
            "actor_bc_lambda": lam}
    m = {"actor_loss": None, "actor_ent": 0.0}
    ag._bc_metrics(m, float(-qmin.sum()), float((d * d).sum()), float(qmin.abs().sum()), 1.0 / B)
    assert list(m) == ["actor_loss", "actor_ent", "actor_bc_loss", "actor_bc_lambda"]
    for k, v in want.items():
        assert m[k] == pytest.approx(v, rel=1e-13)
    mt = {}
    ag._bc_metrics(mt, -qmin.sum().float(), (d * d).sum().float(), qmin.abs().sum().float(), 1.0 / B)
    for k, v in want.items():
        assert torch.is_tensor(mt[k]) and mt[k].dim() == 0 and float(mt[k]) == pytest.approx(v, rel=1e-5)
    assert math.isfinite(float(mt["actor_loss"]))
