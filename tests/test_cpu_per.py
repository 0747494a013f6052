"""Prioritized replay: everything that needs no GPU.  The numpy restatement of the sum tree (tests/per_oracle.py) against an
independent statement of proportional sampling (a cumulative sum and a binary search), the property the descent rule is
there for (it never ends on a zero leaf), the weighted critic step's restatement against the plain oracle and against
autograd, and the public surface (prototypes, header, ABI version, keywords)."""
import inspect
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib, synth
from oracle import drq_oracle as O
from tests import per_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def int_leaves(r, L, kind):
    v = r.randint(1, 50, L).astype(np.float64)
    if kind == "runs":                         # long runs of zero leaves
        for _ in range(3):
            a = r.randint(0, L)
            v[a:a + r.randint(1, L + 1)] = 0
    elif kind == "sparse":
        v[r.uniform(size=L) < 0.8] = 0
    elif kind == "single":
        v[:] = 0
        v[r.randint(0, L)] = r.randint(1, 50)
    elif kind == "last":                       # the only non-zero leaf in the last slot
        v[:] = 0
        v[L - 1] = 7
    if not v.any():
        v[r.randint(0, L)] = 3
    return v


@pytest.mark.parametrize("kind", ["dense", "runs", "sparse", "single", "last"])
def test_descent_equals_cumsum_searchsorted_on_integer_leaves(kind):
    """small-integer leaves: every sum in the tree and in the cumulative sum is exact, so the two statements of
    'the slot whose interval of the total mass holds m' must agree for every row, not nearly"""
    r = np.random.RandomState(5 + len(kind) + ord(kind[0]))
    for trial in range(80):
        L = int(2 ** r.randint(0, 9))
        B = int(r.choice([1, 2, 7, 64, 100]))
        leaves = int_leaves(r, L, kind)
        tree = P.build(leaves)
        assert tree[1] == leaves.sum()
        # u with few mantissa bits and B a small integer: (i + u) / B * total is then compared with integers only
        u = r.randint(0, 1024, B) / 1024.0
        got = P.descend(tree, u)
        m = (np.arange(B) + u) / B * leaves.sum()
        want = np.searchsorted(np.cumsum(leaves), m, side="right")
        assert np.array_equal(got, want), (kind, trial, L, B)
        assert (leaves[got] > 0).all()


def test_descent_never_returns_a_zero_leaf():
    """float leaves from 1e-12 to 1e6 with zeros mixed in, where the inner sums round: u at 0, at the last double
    below 1 and on stratum boundaries; whatever the rounding does to m, the rule may not step into an empty subtree"""
    r = np.random.RandomState(11)
    for trial in range(300):
        L = int(2 ** r.randint(1, 11))
        leaves = 10.0 ** r.uniform(-12, 6, L)
        leaves[r.uniform(size=L) < r.choice([0.0, 0.3, 0.9, 0.99])] = 0.0
        if trial % 7 == 0:
            leaves[L // 2:] = 0.0
        if not leaves.any():
            leaves[r.randint(0, L)] = 1e-12
        tree = P.build(leaves)
        B = int(r.choice([1, 3, 64, 257]))
        for u in (np.zeros(B), np.full(B, np.nextafter(1.0, 0.0)), r.uniform(size=B),
                  np.where(np.arange(B) % 2 == 0, 0.0, np.nextafter(1.0, 0.0))):
            pos = P.descend(tree, u)
            assert pos.min() >= 0 and pos.max() < L
            assert (leaves[pos] > 0).all(), (trial, L, B)
            w = P.weights(tree, pos, int((leaves > 0).sum()), 0.4)
            assert w.max() == 1.0 and (w > 0).all() and np.isfinite(w).all()


def test_fill_and_update_keep_every_inner_node_the_sum_of_its_children():
    r = np.random.RandomState(3)
    tree = P.new_tree(300)
    L = tree.size // 2
    assert L == 512 and tree[0] == 1.0
    P.fill(tree, 10, 200, 1)
    P.fill(tree, 50, 60, 0)
    P.fill(tree, 7, 7, 1)                                          # lo == hi: nothing
    pos = r.randint(10, 200, 64)
    pos[0] = pos[5] = pos[63]                                      # one position in rows 0, 5 and B-1
    td = r.uniform(0, 3, 64).astype(np.float32)
    written = P.update(tree, pos, td, 0.6, 1e-6)
    assert tree[L + pos[63]] == (np.float64(td[63]) + 1e-6) ** 0.6  # the highest row won
    assert tree[0] == max(1.0, max(written.values()))
    k = np.arange(1, L)
    assert np.array_equal(tree[k], tree[2 * k] + tree[2 * k + 1])
    assert tree[L + 55] == 0.0 and tree[L + 5] == 0.0 and tree[L + 250] == 0.0


# ------------------------------------------------------------------------------------------------ weighted critic step
CFG = dict(C=9, A=3, F=20, H=64, B=6, lr=1e-3, sched="0.2", wseed=3, bseed=30)


def oracle(cls, dtype=torch.float64):
    enc, actor, critic = synth.make_weights(CFG["C"], CFG["A"], CFG["F"], CFG["H"], CFG["wseed"])
    return cls(enc, actor, critic, CFG["lr"], stddev_schedule=CFG["sched"], dtype=dtype)


def inputs(u=0):
    batch = synth.make_batch(CFG["B"], CFG["A"], CFG["C"], seed=CFG["bseed"] + u, smooth=True)
    return batch, synth.make_draws(CFG["B"], CFG["A"], seed=CFG["bseed"] + u)


def test_unit_weights_reproduce_the_plain_oracle_exactly():
    plain, per = oracle(O.OracleAgent), oracle(P.PEROracleAgent)
    for u in range(2):
        batch, draws = inputs(u)
        m0 = plain.update(batch, 2 * u, *draws, keep=True)
        m1 = per.update(batch, 2 * u, *draws, weights=torch.ones(CFG["B"]))
        assert m0 == m1
        for key in ("g_enc", "g_critic", "g_actor"):
            for k in plain.last[key]:
                assert torch.equal(plain.last[key][k], per.last[key][k]), (u, key, k)
        for name in ("enc", "actor", "critic", "critic_target"):
            for k, v in getattr(plain, name).items():
                assert torch.equal(v, getattr(per, name)[k]), (u, name, k)
        y, q1, q2 = per.last["target_q"], per.last["q1"], per.last["q2"]
        assert torch.equal(per.last["td_abs"], (0.5 * ((q1 - y).abs() + (q2 - y).abs())).reshape(-1))


def test_closed_form_dq_agrees_with_autograd_for_random_weights():
    per, plain = oracle(P.PEROracleAgent), oracle(O.OracleAgent)
    batch, draws = inputs()
    w = torch.from_numpy(np.random.RandomState(1).uniform(0.25, 1.0, CFG["B"]))
    m = per.update(batch, 0, *draws, weights=w)
    m0 = plain.update(batch, 0, *draws, keep=True)
    L = per.last
    dq1, dq2 = P.closed_form_dq(L["q1"], L["q2"], L["target_q"], w)
    assert torch.allclose(dq1, L["dq1"], rtol=1e-14, atol=0) and torch.allclose(dq2, L["dq2"], rtol=1e-14, atol=0)
    # the loss by the definition, from the plain oracle's intermediates; the unweighted metrics do not move
    y, q1, q2 = plain.last["target_q"], plain.last["q1"], plain.last["q2"]
    want = float((w[:, None] * (q1 - y) ** 2).mean() + (w[:, None] * (q2 - y) ** 2).mean())
    assert m["critic_loss"] == pytest.approx(want, rel=1e-13) and m["critic_loss"] < m0["critic_loss"]
    for k in ("batch_reward", "critic_target_q", "critic_q1", "critic_q2"):
        assert m[k] == m0[k]
    assert list(m) == list(m0)


# ------------------------------------------------------------------------------------------------ public surface
NEW = ("drq_per_fill", "drq_per_sample", "drq_per_update", "drq_td_mse_w", "drq_update_phase_per")


def test_prototypes_header_and_abi_version():
    with open(os.path.join(ROOT, "include", "drqv2_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert f"int {name}(" in header, name
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()
    assert len(_lib.DrqStep._fields_) == 40                        # the descriptor did not grow
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.load().drq_abi_version() == 7
    from drqv2_amd import build
    assert "per.hip" in build.SOURCES


def test_keywords_and_refusals_without_a_gpu():
    import drqv2
    import replay_buffer as rb
    from drqv2_amd.engine import StepEngine
    from drqv2_amd.replay import DeviceReplay, IndexedBatch, PrioritizedBatch
    for fn in (DeviceReplay.__init__, rb.make_replay_loader):
        ps = inspect.signature(fn).parameters
        assert ps["priority_alpha"].default is None and ps["priority_beta"].default == 0.4
        assert ps["priority_eps"].default == 1e-6
    assert inspect.signature(StepEngine.update).parameters["loss_weights"].default is None
    assert callable(PrioritizedBatch.update_priorities) and IndexedBatch is not PrioritizedBatch
    # None is the store as it was: no tree, and the RandomState is consumed as before
    rp = DeviceReplay(50, (9, 84, 84), 2, 3, 0.99, "cpu", seed=4)
    assert rp.tree is None and rp.priority_alpha is None
    for bad in (0.0, -0.5, 1.5, float("nan"), True):
        with pytest.raises(ValueError):
            DeviceReplay(50, (9, 84, 84), 2, 3, 0.99, "cpu", seed=4, priority_alpha=bad)
    with pytest.raises(_lib.DrqError, match="GPU"):
        DeviceReplay(50, (9, 84, 84), 2, 3, 0.99, "cpu", seed=4, priority_alpha=0.6)
    # the engine's refusals come before anything is launched
    ag = drqv2.DrQV2Agent((9, 84, 84), (3,), "cpu", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, False)
    eng = ag._engine
    w = torch.ones(4)
    with pytest.raises(_lib.DrqError, match="shape"):
        eng._loss_weights(torch.ones(5), 4)
    with pytest.raises(_lib.DrqError, match="float32"):
        eng._loss_weights(torch.ones(4, dtype=torch.float64), 4)
    ag.set_behavior_cloning(2.5)
    with pytest.raises(_lib.DrqError, match="behaviour cloning"):
        eng._loss_weights(w, 4)
    ag.set_behavior_cloning(None)
    ag.set_compute_dtype("bf16")
    with pytest.raises(_lib.DrqError, match="bf16"):
        eng._loss_weights(w, 4)
    ag.set_compute_dtype("fp32")
    eng.pg = object()
    with pytest.raises(_lib.DrqError, match="data parallelism"):
        eng._loss_weights(w, 4)
    eng.pg = None
    assert eng._loss_weights(w, 4)[1].shape == (4,)
    ptrs = [eng._loss_weights(w, 4)[1].data_ptr() for _ in range(5)]
    assert len(set(ptrs[:4])) == 4 and ptrs[4] == ptrs[0]          # four td_abs buffers, used in turn
