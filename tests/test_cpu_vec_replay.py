"""Step-major replay (VecDeviceReplay, drq_vec_add / drq_vec_sample): everything that needs no GPU.  The public surface
(header, prototype table, build list, ABI version), the numpy restatement tests/vec_oracle.py -- its bounds and slot
arithmetic, its candidate choice, and its windows against oracle.nstep_sample on columns built by hand -- and the
argument errors and the CPU refusal of the store."""
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from oracle import drq_oracle as O
from tests import abi
from tests import vec_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("drq_vec_add", "drq_vec_sample")


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_build_list_and_abi_version():
    for name in NEW:
        abi.assert_prototype(name)
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()        # additive: the version stays
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.drq_abi_version() == 7
        # argument errors are reported before any launch: no GPU needed
        assert lib.drq_vec_add(*([None] * 5), 16, 3, 2, 16, 0, *([None] * 5), None) == -1
        assert lib.drq_vec_sample(*([None] * 4), 16, 3, 2, 16, 1, 4, None, 8, 4, 3, 0.99, *([None] * 8), None) == -1
    from drqv2_amd import build
    assert "vecreplay.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "vecreplay.hip"))


# ------------------------------------------------------------------------------------------------ the restatement
def test_bounds_and_slots():
    R, N, nstep, guard = 16, 3, 3, 8
    # T < R: nothing has been overwritten yet; the head keeps nstep rows back, and lo leaves 1 as soon as `guard` more
    # rows could overwrite row lo - 1
    assert V.bounds(7, R, nstep, guard) == (1, 4)
    assert V.bounds(10, R, nstep, guard) == (3, 7)
    assert V.bounds(2, R, nstep, guard) == (1, -1)                       # hi < lo: nothing to draw yet
    assert V.bounds(R - guard, R, nstep, guard) == (1, R - guard - nstep)
    # T = R: the ring is full, the next add overwrites row 0; lo already keeps guard rows (+ row t-1) clear of the head
    assert V.bounds(R, R, nstep, guard) == (1 + guard, R - nstep)
    # T = 3R + 1
    T = 3 * R + 1
    lo, hi = V.bounds(T, R, nstep, guard)
    assert (lo, hi) == (T - R + 1 + guard, T - nstep) == (42, 46)
    for T in (10, R, 3 * R + 1, 1000):
        lo, hi = V.bounds(T, R, nstep, guard)
        assert hi - lo + 1 + nstep <= R                                  # rows lo-1 .. hi+nstep-1: distinct ring rows
        # ... and they stay that while up to `guard` more rows are added: the oldest row read is lo-1 >= T+guard-R
        assert lo - 1 >= T + guard - R
        assert len({V.slot(t, 0, R, N) for t in range(lo - 1, hi + nstep)}) == hi + nstep - lo + 1
    assert V.slot(0, 0, R, N) == 0 and V.slot(1, 2, R, N) == 5 and V.slot(R, 1, R, N) == 1
    assert V.slot(3 * R + 1, 2, R, N) == N + 2 and V.slot(R + 2, 0, R, N) == 2 * N
    assert sorted(V.slot(t, e, R, N) for t in range(R, 2 * R) for e in range(N)) == list(range(R * N))


def column(T, N, A, resets, seed, fb=16, zero_disc=()):
    """T rows of N environments; resets: {env: rows with first = 1} (row 0 always)"""
    r = np.random.RandomState(seed)
    rows = []
    for t in range(T):
        first = np.array([t == 0 or t in resets.get(e, ()) for e in range(N)], np.uint8)
        disc = np.array([0.0 if (t, e) in zero_disc else 1.0 for e in range(N)], np.float32)
        rows.append((r.randint(0, 256, (N, fb)).astype(np.uint8), r.uniform(-1, 1, (N, A)).astype(np.float32),
                     r.randn(N).astype(np.float32), disc, first))
    return rows


def u_for(targets, lo, hi, N, K=4):
    """a u row whose candidates are the given (t, e), repeated to K"""
    M = (hi - lo + 1) * N
    t = list(targets) + [targets[-1]] * (K - len(targets))
    return [(((tt - lo) * N + e) + 0.5) / M for tt, e in t]


@pytest.mark.parametrize("nstep,gamma", [(1, 0.99), (3, 0.99), (5, 0.9)])
def test_windows_equal_nstep_sample_with_a_reset_at_every_offset(nstep, gamma):
    """one environment, a reset placed i rows behind the drawn transition for i = 1 .. nstep + 1: the window has
    min(i, nstep) steps and equals oracle.nstep_sample on an episode dict built here from the raw rows, and the plain
    float32 loop written out once more"""
    R, A, t0 = 32, 2, 4
    for off in range(1, nstep + 2):
        rows = column(20, 1, A, {0: (2, t0 + off)}, seed=off, zero_disc={(t0 + off - 1, 0)} if off % 2 else ())
        vo = V.VecOracle(R, 1, A, 16, nstep, gamma, guard_rows=0)
        for row in rows:
            vo.add(*row)
        lo, hi = vo.bounds()
        assert (lo, hi) == (1, 20 - nstep)
        got = vo.sample(np.array([u_for([(t0, 0)], lo, hi, 1)]))
        k = min(off, nstep)
        assert got["rows"] == [(t0, 0)] and got["steps"][0] == k
        assert got["tally"] == {"accept0": 1, ("full" if k == nstep else f"cut{k}"): 1}
        assert got["idx"][:, 0].tolist() == [t0 - 1, t0 + k - 1, t0]
        ep = {"observation": np.stack([rw[0][0] for rw in rows[2:t0 + off]]),
              "action": np.stack([rw[1][0] for rw in rows[2:t0 + off]]),
              "reward": np.stack([rw[2][:1] for rw in rows[2:t0 + off]]),
              "discount": np.stack([rw[3][:1] for rw in rows[2:t0 + off]])}
        o, a, rr, dd, n = O.nstep_sample(ep, t0 - 2, k, gamma)
        assert np.array_equal(got["obs"][0], o) and np.array_equal(got["next_obs"][0], n)
        assert np.array_equal(got["action"][0], a)
        assert got["reward"][0].tobytes() == rr[0].tobytes() and got["discount"][0].tobytes() == dd[0].tobytes()
        acc_r, acc_d = np.float32(0), np.float32(1)
        for i in range(k):
            acc_r = np.float32(acc_r + np.float32(acc_d * rows[t0 + i][2][0]))
            acc_d = np.float32(acc_d * np.float32(rows[t0 + i][3][0] * np.float32(gamma)))
        assert got["reward"][0] == acc_r and got["discount"][0] == acc_d
        assert np.array_equal(got["obs"][0], rows[t0 - 1][0][0]) and np.array_equal(got["next_obs"][0], rows[t0 + k - 1][0][0])


def test_candidate_choice_rejection_walk_and_empty_environment():
    R, N, A, nstep = 16, 3, 2, 3
    T = 2 * R + 5
    lo, hi = V.bounds(T, R, nstep, 0)
    assert (lo, hi) == (22, 34)
    rows = column(T, N, A, {1: (lo + 2, lo + 3, hi - 1, hi), 2: range(T)}, seed=1)
    vo = V.VecOracle(R, N, A, 16, nstep, 0.99, guard_rows=0)
    for row in rows:
        vo.add(*row)
    u = np.array([u_for([(lo, 0)], lo, hi, N),
                  u_for([(lo, 2), (lo + 1, 0)], lo, hi, N),
                  u_for([(lo, 2), (hi, 2), (lo + 5, 2), (lo + 4, 1)], lo, hi, N),
                  u_for([(lo + 2, 1), (lo, 2)], lo, hi, N),
                  u_for([(hi - 1, 1), (lo, 2)], lo, hi, N),
                  u_for([(lo + 7, 2)], lo, hi, N)])
    got = vo.sample(u)
    assert got["rows"] == [(lo, 0), (lo + 1, 0), (lo + 4, 1), (lo + 4, 1), (lo, 1), (lo + 7, 2)]
    assert got["steps"].tolist() == [3, 3, 3, 3, 2, 0]                # (lo, 1): the reset at lo + 2 cuts it
    t = got["tally"]
    assert (t["accept0"], t["accept1"], t["accept3"], t["walk"], t["walk_wrap"], t["empty"]) == (1, 1, 1, 1, 1, 1)
    assert t["cut2"] == 1 and t["full"] == 4
    s = V.slot(lo + 7, 2, R, N)
    assert got["idx"][:, 5].tolist() == [s, s, s] and got["reward"][5] == 0 and got["discount"][5] == 0
    # u = 0 is the first cell, the last double below 1 the last one (the min() of the contract never binds below 2^53)
    assert vo.choose([0.0] * 4)[:2] == (lo, 0) and vo.choose([np.nextafter(1.0, 0.0)] * 4) == (hi, 2, 0, "empty")
    ring, written = vo.ring()
    assert written.all() and ring["first"][V.slot(hi, 1, R, N)] == 1 and ring["first"][V.slot(lo, 1, R, N)] == 0
    assert np.array_equal(ring["frames"][V.slot(T - 1, 0, R, N)], rows[T - 1][0][0])


# ------------------------------------------------------------------------------------------------ the store, no GPU
def test_constructor_and_add_argument_errors_and_cpu_refusal():
    from drqv2_amd.replay import VecDeviceReplay
    OBS = (1, 4, 4)
    mk = lambda **kw: VecDeviceReplay(**{**dict(rows=16, num_envs=3, obs_shape=OBS, action_dim=2, nstep=3, discount=0.99,
                                                device="cpu", seed=0), **kw})
    for bad in (dict(rows=12), dict(rows=14, guard_rows=10), dict(num_envs=0), dict(obs_shape=(1, 3, 5)), dict(nstep=0),
                dict(action_dim=0)):
        with pytest.raises(ValueError):
            mk(**bad)
    st = mk(rows=13)                                                      # nstep + guard_rows + 2
    assert st.guard_rows == 8 and st.indexed is True and len(st) == 0 and st.bounds() == (1, -3)
    assert mk(rows=7, guard_rows=2).R == 7
    N, A = 3, 2
    obs, act = np.zeros((N,) + OBS, np.uint8), np.zeros((N, A), np.float32)
    rew, disc, first = np.zeros(N, np.float32), np.ones((N, 1), np.float32), np.zeros(N, bool)
    for bad in ((obs[:2], act, rew, disc, first), (obs.astype(np.float32), act, rew, disc, first),
                (obs, act[:, :1], rew, disc, first), (obs, act.astype(np.int32), rew, disc, first),
                (obs, act, np.zeros((N, 2), np.float32), disc, first), (obs, act, rew, disc[:2], first),
                (obs, act, rew, disc, np.zeros((N, 1), bool)), (obs, act, rew, disc, np.zeros(N, np.float32)),
                (obs.tolist(), act, rew, disc, first), (torch.zeros((N, 17), dtype=torch.uint8), act, rew, disc, first)):
        with pytest.raises(ValueError):
            st.add(*bad)
    assert st.T == 0
    # well-formed rows on a CPU store: refused like the rest of the device replay, nothing is counted
    for good in ((obs, act, rew, disc, first), (torch.from_numpy(obs).view(N, 16), act.astype(np.float64), rew[:, None], disc, None)):
        with pytest.raises(_lib.DrqError, match="no CPU fallback"):
            st.add(*good)
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        st.sample(4)
    assert st.T == 0 and st.last_steps is None
    from drqv2_amd.replay import BatchIterator
    assert isinstance(iter(st), BatchIterator)
