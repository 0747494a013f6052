"""Demonstrations in the step-major replay (VecDeviceReplay(demo_rows=D), drq_vec_sample_mixed): everything that needs
no GPU.  The public surface of the new entry, the constructor's refusals, demo_fraction and the split of a batch, the
saved state of stores with and without a partition, and the numpy restatement tests/vec_demo_oracle.py on the partition
it builds."""
import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from drqv2_amd.replay import VecDeviceReplay, VecFrameReplay
from tests import abi
from tests import vec_demo_oracle as M

NAME = "drq_vec_sample_mixed"
R, D, N, A, FB, NSTEP = 12, 9, 3, 2, 16, 3


def store(demo_rows=D, **kw):
    kw.setdefault("seed", 1)
    return VecDeviceReplay(R, N, (FB,), A, NSTEP, 0.99, "cpu", guard_rows=2, demo_rows=demo_rows, **kw)


# ------------------------------------------------------------------------------------------------ public surface
def test_entry_is_declared_on_both_sides_and_refuses_before_any_launch():
    abi.assert_prototype(NAME)
    assert len(_lib.PROTOTYPES[NAME][1]) == 27 and NAME not in _lib.NO_STREAM and NAME in abi.stream_entries()
    lib = _lib.load()
    assert lib.drq_abi_version() == 7                                   # additive: the version stays
    # no GPU needed: the check precedes the launch
    assert lib.drq_vec_sample_mixed(*([None] * 4), R, D, N, A, FB, 1, 4, 8, None, 7, 3, 4, NSTEP, 0.99, *([None] * 8),
                                    None) == -1


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_refusals_each_say_why(monkeypatch):
    with pytest.raises(ValueError, match=r"demo_rows 4: at least nstep \+ 2 = 5"):
        store(demo_rows=NSTEP + 1)
    with pytest.raises(ValueError, match="at least nstep"):
        store(demo_rows=-1)
    assert store(demo_rows=NSTEP + 2).D == NSTEP + 2
    with pytest.raises(ValueError, match="priority_alpha: the sum tree covers the ring only"):
        store(priority_alpha=0.6)
    # the slot bound: 3 * (R + D) * N must fit the int the fused aug+conv1 launch casts 3 * slot + g to.  Refused before
    # anything is allocated (this store would take 20 GB) ...
    with pytest.raises(ValueError, match=r"32-bit index 3 \* slot \+ g"):
        VecDeviceReplay(16, 2 ** 26, (FB,), A, NSTEP, 0.99, "cpu", demo_rows=16)
    # ... and exact at the edge, shown on a small store by moving the limit
    assert VecDeviceReplay.MAX_INDEXED_UNITS == 2 ** 31 - 1
    monkeypatch.setattr(VecDeviceReplay, "MAX_INDEXED_UNITS", 3 * (R + D) * N)
    assert store().D == D
    monkeypatch.setattr(VecDeviceReplay, "MAX_INDEXED_UNITS", 3 * (R + D) * N - 1)
    with pytest.raises(ValueError, match=f"= {(R + D) * N} slots"):
        store()
    assert store(demo_rows=0).D == 0                                    # a store without demonstrations has no such bound


def test_single_frame_ring_refuses_demonstrations():
    with pytest.raises(ValueError, match="single-frame ring holds no demonstrations"):
        VecFrameReplay(16, N, A, NSTEP, 0.99, "cpu", demo_rows=D)
    assert VecFrameReplay(16, N, A, NSTEP, 0.99, "cpu", demo_rows=0).D == 0


def test_layout_ring_views_and_partition_share_one_allocation():
    st = store()
    S = R * N
    for n in VecDeviceReplay._RING:
        whole, ring, part = st._whole[n], getattr(st, n), st._demo[n]
        assert whole.shape[0] == (R + D) * N and ring.shape[0] == S and part.shape[0] == D * N
        assert ring.data_ptr() == whole.data_ptr()
        assert part.data_ptr() == whole.data_ptr() + S * whole.stride(0) * whole.element_size()
    assert st.demo_rows_filled == 0 and st.demo_bounds() == (1, -NSTEP) and st.last_demo_count == 0
    plain = store(demo_rows=0)
    assert all(plain._whole[n] is getattr(plain, n) for n in VecDeviceReplay._RING)     # the allocation itself, as before
    assert plain.frames.shape[0] == S


# ------------------------------------------------------------------------------------------------ demo_fraction
def test_demo_fraction_is_validated_and_splits_the_batch():
    st = store()
    assert st.demo_fraction == 0.0
    for f, bd in ((0, 0), (0.07, 0), (0.5, 4), (1, 7)):
        st.demo_fraction = f
        assert st.demo_fraction == float(f) and st.demo_count(7) == bd == int(7 * f + 0.5)
    for bad in (-0.01, 1.0001, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="a float in"):
            st.demo_fraction = bad
        assert st.demo_fraction == 1.0                                  # unchanged by a refused value
    plain = store(demo_rows=0)
    plain.demo_fraction = 0.0
    with pytest.raises(ValueError, match="no demonstration partition"):
        plain.demo_fraction = 0.5
    with pytest.raises(ValueError, match="no demonstration partition"):
        plain.add_demonstrations([])


def test_no_cpu_fallback_and_overfull_partition_refused_first():
    st = store()
    r = np.random.RandomState(0)
    ep = lambda n: {"observation": r.randint(0, 256, (n + 1, FB)).astype(np.uint8),
                    "action": r.uniform(-1, 1, (n + 1, A)).astype(np.float32),
                    "reward": r.randn(n + 1, 1).astype(np.float32), "discount": np.ones((n + 1, 1), np.float32)}
    with pytest.raises(ValueError, match=r"need L = 10 rows per lane behind the 0 already filled.*demo_rows = 9"):
        st.add_demonstrations([ep(9), ep(2), ep(2)])
    with pytest.raises(ValueError, match=r"add_demonstrations\(\): episode 1: action"):
        st.add_demonstrations([ep(2), dict(ep(2), action=np.zeros((3, A + 1), np.float32))])
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        st.add_demonstrations([ep(2)])
    assert st.demo_rows_filled == 0


# ------------------------------------------------------------------------------------------------ checkpoints
def keys_of(sd):
    return set(sd), set(sd["config"])


def test_state_of_a_store_without_demonstrations_has_no_new_key():
    top, cfg = keys_of(store(demo_rows=0).state_dict())
    assert top == {"format", "kind", "config", "T", "priority_beta", "live_slots", "ring", "rng", "frames", "action",
                   "reward", "discount", "first"}
    assert cfg == {"R", "N", "A", "slot_shape", "nstep", "gamma", "guard_rows", "indexed", "priority_alpha", "priority_eps"}
    top_d, cfg_d = keys_of(store().state_dict())
    assert top_d - top == {"demo_rows_filled", "demo_fraction", "demos"} and cfg_d - cfg == {"demo_rows"}
    assert "demos" not in store().state_dict(frames=False)


def filled(seed, Td=5, fraction=0.25):
    """a CPU store whose partition holds Td rows written by hand (add_demonstrations needs the GPU)"""
    st = store(seed=seed)
    g = torch.Generator().manual_seed(seed)
    n = Td * N
    st._demo["frames"][:n] = torch.randint(0, 256, (n, FB), dtype=torch.uint8, generator=g)
    st._demo["action"][:n] = torch.rand((n, A), generator=g)
    st._demo["reward"][:n] = torch.randn(n, generator=g)
    st._demo["discount"][:n] = 0.5
    st._demo["first"][:n] = torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g)
    st.demo_rows_filled, st.demo_fraction = Td, fraction
    st.rng.random_sample(3)
    return st


def same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "demos":
            assert set(a[k]) == set(b[k]) and all(torch.equal(a[k][n], b[k][n]) for n in a[k])
        elif k == "rng":
            assert a[k][0] == b[k][0] and torch.equal(a[k][1], b[k][1]) and tuple(a[k][2:]) == tuple(b[k][2:])
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_state_with_demonstrations_round_trips_on_a_cpu_store():
    src = filled(3)
    sd = src.state_dict()
    assert sd["demo_rows_filled"] == 5 and sd["demo_fraction"] == 0.25 and sd["config"]["demo_rows"] == D
    assert sd["demos"]["frames"].shape == (5 * N, FB) and sd["demos"]["first"].dtype == torch.uint8
    dst = filled(4, Td=7, fraction=1.0)                                 # a used store: everything it held is replaced
    dst.load_state_dict(sd)
    same_state(dst.state_dict(), sd)
    assert dst.demo_rows_filled == 5 and dst.demo_fraction == 0.25 and dst.demo_bounds() == (1, 5 - NSTEP)
    for n in VecDeviceReplay._RING:
        assert torch.equal(dst._whole[n], src._whole[n]), n             # the slots above Td N are the constructor's again
    # nothing changes on an error: a partition array of another shape, a Td the partition cannot hold, no demonstrations
    before = dst.state_dict()
    for breaker, msg in ((lambda s: s["demos"].update(action=s["demos"]["action"][:-1]), "demos.action"),
                         (lambda s: s.update(demo_rows_filled=D + 1), "do not fit a partition of 9 rows"),
                         (lambda s: s.update(demo_fraction=1.5), "do not fit a partition"),
                         (lambda s: s.pop("demos"), "holds no demonstrations")):
        bad = dict(filled(5, Td=2).state_dict())
        bad["demos"] = dict(bad["demos"])
        breaker(bad)
        with pytest.raises(ValueError, match=msg):
            dst.load_state_dict(bad)
        same_state(dst.state_dict(), before)
    # frames=False: Td and the fraction travel, the arrays stay
    light = filled(6, Td=5, fraction=0.75).state_dict(frames=False)
    dst.load_state_dict(light, frames=False)
    assert dst.demo_fraction == 0.75 and torch.equal(dst._demo["frames"], src._demo["frames"])


def test_configuration_mismatch_on_demo_rows_is_named_both_ways():
    with_d, without = store().state_dict(), store(demo_rows=0).state_dict()
    with pytest.raises(ValueError, match="demo_rows: saved 9, here 0"):
        store(demo_rows=0).load_state_dict(with_d)
    with pytest.raises(ValueError, match="demo_rows: saved '<absent>', here 9"):
        store().load_state_dict(without)
    with pytest.raises(ValueError, match="demo_rows: saved 9, here 8"):
        store(demo_rows=8).load_state_dict(with_d)
    store(demo_rows=0).load_state_dict(without)                         # and what fitted before still does


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n_envs", [1, 3])
@pytest.mark.parametrize("nstep", [1, 3])
def test_oracle_partition_meets_every_branch_and_offsets_its_indices(n_envs, nstep):
    mo = M.MixedOracle(R, D, n_envs, A, FB, nstep, 0.99, guard_rows=0)
    M.fill_partition(mo, seed=1)
    assert mo.Td == M.TD == 8 and mo.demo_bounds() == (1, 8 - nstep)
    r = np.random.RandomState(2)
    for t in range(2 * R + 5):
        mo.add(r.randint(0, 256, (n_envs, FB)), r.uniform(-1, 1, (n_envs, A)), r.randn(n_envs), np.ones(n_envs),
               r.uniform(size=n_envs) < 0.2)
    rows = M.crafted_rows(mo)
    u = np.concatenate([np.array(rows), r.random_sample((7 - len(rows), 4))])
    with pytest.raises(AssertionError, match="never took"):
        mo.require_branches(empty=n_envs == 3)                          # nothing drawn yet: the check can fail
    want = mo.sample(u, len(rows))
    mo.require_branches(empty=n_envs == 3)
    assert want["idx"].shape == (3, 7) and (want["idx"][:, :len(rows)] >= R * n_envs).all()
    whole = mo.whole()
    assert whole["frames"].shape == ((R + D) * n_envs, FB)
    # the frames of a materialised batch are the whole allocation's at the indices, partition rows included
    assert np.array_equal(whole["frames"][want["idx"][0]], want["obs"])
    assert np.array_equal(whole["frames"][want["idx"][1]], want["next_obs"])
    assert np.array_equal(whole["action"][want["idx"][2]], want["action"])
    if n_envs == 3:
        b = len(rows) - 1                                               # the lane of reset rows: steps 0, all on one slot
        assert want["steps"][b] == 0 and len(set(want["idx"][:, b])) == 1 and want["reward"][b] == 0 == want["discount"][b]
    # Bd = 0 and Bd = B are the two plain draws
    assert np.array_equal(mo.sample(u, 0)["idx"], mo.live.sample(u)["idx"])
    assert np.array_equal(mo.sample(u, 7)["idx"], mo.demo.sample(u)["idx"] + R * n_envs)
