"""Prioritized sampling on the step-major ring (VecDeviceReplay(priority_alpha=...), drq_vec_per_advance / _sample /
_update): everything that needs no GPU.  The public surface (header, prototype table, exports, ABI version), the argument
errors of the three entries and of the constructor, and the numpy restatement tests/vec_per_oracle.py on its own: the
invariant of the tree through three wraps of the ring, the recovery of a row from its slot, the uniform limit of the draw."""
import os

import numpy as np
import pytest

from drqv2_amd import _lib
from tests import abi
from tests import per_oracle as P
from tests import vec_oracle as V
from tests import vec_per_oracle as VP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("drq_vec_per_advance", "drq_vec_per_sample", "drq_vec_per_update")
EARG = -1


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_exports_and_abi_version():
    for name in NEW:
        abi.assert_prototype(name)
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()        # additive: the version stays
    lib = _lib.load()
    assert lib.drq_abi_version() == 7
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"


def test_entries_refuse_null_pointers_before_any_launch():
    """argument errors are reported before a launch: no GPU needed.  Every pointer NULL, then every other argument sound"""
    lib = _lib.load()
    R, N, A, L, T, lo, hi, B, nstep = 16, 3, 2, 64, 40, 27, 37, 8, 3
    assert lib.drq_vec_per_advance(None, L, None, R, N, T, 37, 26, None) == EARG
    assert lib.drq_vec_per_sample(None, L, None, None, None, None, R, N, A, T, lo, hi, None, B, nstep, 0.99, 0.4,
                                  *([None] * 6), None) == EARG
    assert lib.drq_vec_per_update(None, L, None, R, N, T, lo, hi, None, None, B, 0.6, 1e-6, None) == EARG


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_argument_errors_and_the_uniform_default():
    from drqv2_amd.replay import VecDeviceReplay
    mk = lambda **kw: VecDeviceReplay(**{**dict(rows=16, num_envs=3, obs_shape=(1, 4, 4), action_dim=2, nstep=3,
                                                discount=0.99, device="cpu", seed=0), **kw})
    for bad in (dict(priority_alpha=0.6, indexed=False), dict(priority_alpha=0.0), dict(priority_alpha=-0.5),
                dict(priority_alpha=float("nan")), dict(priority_alpha=float("inf")), dict(priority_alpha=True),
                dict(priority_alpha=0.6, priority_beta=-0.1), dict(priority_alpha=0.6, priority_beta=float("nan")),
                dict(priority_alpha=0.6, priority_eps=-1e-6), dict(priority_alpha=0.6, priority_eps=float("nan"))):
        with pytest.raises(ValueError):
            mk(**bad)
    # the tree lives on the GPU: a sound prioritized store on the CPU is refused like DeviceReplay's
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        mk(priority_alpha=0.6)
    st = mk()
    assert st.tree is None and st.priority_alpha is None and st.priority_beta == 0.4 and st.priority_eps == 1e-6
    assert mk(indexed=False, priority_beta=0.7).priority_beta == 0.7      # without alpha the other two are only kept


# ------------------------------------------------------------------------------------------------ the restatement
R, N, A, FB, NSTEP, GUARD = 16, 3, 2, 16, 3, 2
# resets (row -> environments): two adjacent reset rows in environment 1, one in every environment at once, and -- below
# -- one on every row that is the entering row of some add (hi = T - nstep covers every row from 1 on)
RESETS = {5: (0,), 9: (1,), 10: (1,), 14: (0, 1, 2), 20: (2,), 21: (0,), 22: (0,), 30: (1,), 31: (2,), 40: (0, 2), 45: (1,)}


def stepped(n_rows, resets=RESETS, guard=GUARD, seed=0):
    """yields the oracle after every add"""
    r = np.random.RandomState(seed)
    vp = VP.VecPEROracle(R, N, A, FB, NSTEP, 0.99, guard_rows=guard)
    for t in range(n_rows):
        first = np.array([e in resets.get(t, ()) for e in range(N)], np.uint8)
        vp.add(r.randint(0, 256, (N, FB)), r.uniform(-1, 1, (N, A)), r.standard_normal(N), np.ones(N), first)
        yield vp


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_invariant_holds_after_every_add_through_three_wraps():
    entered_a_reset = 0
    for vp in stepped(3 * R + 1):
        T = vp.T
        lo, hi = vp.bounds()
        t, L = vp.tree, vp.L
        want = np.zeros(L, bool)                                   # from the definition, not from the oracle's helper
        for tt in range(lo, hi + 1):
            for e in range(N):
                want[V.slot(tt, e, R, N)] = vp.vo.first[tt][e] == 0
        assert np.array_equal(t[L:] > 0, want), T
        assert (t[L:][~want] == 0).all() and (t[L + R * N:] == 0).all()
        assert np.array_equal(want, vp.expected_leaf_mask())
        k = np.arange(1, L)
        assert np.array_equal(bits(t[k]), bits(t[2 * k] + t[2 * k + 1])), T     # every inner node: left + right, bitwise
        assert t[0] == 1.0 and (t[L:][want] == 1.0).all()          # no update yet: everything at the initial maximum
        if hi >= lo:
            entered_a_reset += int(vp.vo.first[hi].any())
        # advance arguments come from the counters alone, and a row leaves exactly when lo has moved
        enter, leave = VP.entering_leaving(T, R, NSTEP, GUARD)
        assert enter == (hi if hi >= lo else -1)
        assert (leave >= 0) == (lo > V.bounds(T - 1, R, NSTEP, GUARD)[0]) and (leave < 0 or leave == lo - 1)
    assert T == 3 * R + 1 and entered_a_reset >= 8


def test_invariant_survives_priority_updates():
    """updates on drawn and on stale positions in between the adds: positive leaves stay where the invariant wants them"""
    r = np.random.RandomState(3)
    held = None
    for vp in stepped(3 * R + 1):
        lo, hi = vp.bounds()
        if hi < lo:
            continue
        if held is not None:                                       # a batch drawn one add ago
            vp.update(held, r.uniform(0, 5, held.size))
        held = vp.sample(r.random_sample(12))["pos"]
        vp.update(np.array([-1, R * N, vp.L, V.slot(hi + 1, 0, R, N), V.slot(lo - 1, 1, R, N)]), np.full(5, 9.0))
        t, L = vp.tree, vp.L
        assert np.array_equal(t[L:] > 0, vp.expected_leaf_mask())
        k = np.arange(1, L)
        assert np.array_equal(bits(t[k]), bits(t[2 * k] + t[2 * k + 1]))
        assert t[0] < (9.0 + 1e-6) ** 0.6                          # the skipped rows did not raise the maximum
    assert vp.tree[0] > 1.0


@pytest.mark.parametrize("T", [1, 7, R, R + 1, 2 * R + 5, 3 * R + 1, 1000])
def test_row_recovery_inverts_the_slot(T):
    for t in range(max(0, T - R), T):
        for e in range(N):
            p = V.slot(t, e, R, N)
            assert VP.row_of(p, T, R, N) == t and p % N == e
    if T < R:                                                      # ring rows never written map below row 0
        assert VP.row_of(V.slot(T, 0, R, N), T, R, N) == T - R < 0


def test_equal_leaves_draw_uniformly_over_the_valid_positions():
    for vp in stepped(2 * R + 5):
        pass
    valid = np.nonzero(vp.expected_leaf_mask())[0]
    lo, hi = vp.bounds()
    assert 0 < valid.size < (hi - lo + 1) * N                       # some drawable rows are reset rows
    B = 4 * valid.size
    got = vp.sample(np.full(B, 0.5))
    assert np.array_equal(np.bincount(got["pos"], minlength=vp.L)[valid], np.full(valid.size, 4))
    assert set(got["pos"].tolist()) == set(valid.tolist())
    assert np.array_equal(got["weights"], np.ones(B))
    for (t, e), k, p in zip(got["rows"], got["steps"], got["pos"]):
        assert lo <= t <= hi and vp.vo.first[t][e] == 0 and 1 <= k <= NSTEP and V.slot(t, e, R, N) == p


def test_empty_tree_rows():
    every = {t: (0, 1, 2) for t in range(64)}
    for vp in stepped(R + 3, resets=every):
        assert vp.tree[1] == 0 and not vp.tree[1:].any()
    lo, hi = vp.bounds()
    got = vp.sample(np.array([0.0, 0.3, 0.999]))
    s = V.slot(lo, 0, R, N)
    assert (got["idx"] == s).all() and (got["steps"] == 0).all() and not got["reward"].any() and not got["discount"].any()
    assert np.array_equal(got["weights"], np.ones(3)) and np.array_equal(got["action"][1], vp.vo.action[lo][0])
    assert vp.update(got["pos"], np.ones(3, np.float32)) == {} and vp.tree[1] == 0 and vp.tree[0] == 1.0


def test_update_clamps_and_keeps_the_highest_row():
    for vp in stepped(2 * R + 5):
        pass
    valid = np.nonzero(vp.expected_leaf_mask())[0]
    a, b, c, d = valid[:4].tolist()
    td = np.array([1.0, np.nan, -3.0, np.inf, 2.0], np.float32)
    written = vp.update(np.array([a, b, c, d, a]), td)
    L = vp.L
    assert written[a] == vp.tree[L + a] == (2.0 + 1e-6) ** 0.6
    assert vp.tree[L + b] == vp.tree[L + c] == (1e-6) ** 0.6
    assert vp.tree[L + d] == vp.tree[0] == (VP.FLT_MAX + 1e-6) ** 0.6 and np.isfinite(vp.tree[1])
    assert P.leaves_of(R * N) == L == 64
