"""The k-NN bonus without a GPU: the numpy oracle (tests/knn_oracle.py) against a scalar float32 loop that follows the
words of the contract (include/drqv2_hip.h, "k-NN bonus"), a check that the GPU tests' inputs tell a contracted build from
a correct one, and the host side of drqv2_amd.explore.KnnBonus / RandomFeatures -- argument checks, the misaligned
observe(), state dicts, the checkpoint file, the registration of the entries.  tests/test_hip_knn.py holds the kernel to
this oracle."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import abi
from tests import knn_oracle as K

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("drq_explore_knn", "drq_explore_knn_ws_bytes")


# ------------------------------------------------------------------------------------------------ registration
def test_entries_are_registered_declared_and_built():
    import drqv2_amd.explore as X
    from drqv2_amd import _lib, build
    assert (X.KNN_MAX_DIM, X.KNN_MAX_K, X.KNN_CHUNK) == (K.MAX_DIM, K.MAX_K, K.CHUNK) == (64, 8, 128)
    assert abi.define("DRQ_KNN_MAX_DIM") == 64 and abi.define("DRQ_KNN_MAX_K") == 8 and abi.define("DRQ_KNN_CHUNK") == 128
    assert "knn.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "knn.hip"))
    assert build.FILE_FLAGS["knn.hip"] == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    for name in NAMES:
        abi.assert_prototype(name)
    assert "drq_explore_knn" not in _lib.NO_STREAM and "drq_explore_knn_ws_bytes" in _lib.NO_STREAM
    assert "drq_explore_knn" in abi.stream_entries()
    hdr = abi.text()
    assert "---- k-NN bonus" in hdr
    for text in ("c = offset + j * stride with c < live", "t = q[i] - x[i];  acc = acc + t * t", "A D that is NaN counts as +infinity",
                 "sqrtf(the k-th smallest D)", "No row >= live is ever read"):
        assert text in hdr, text
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    for name in NAMES:
        assert hasattr(_lib.load(), name)


def test_refusals_and_the_workspace_size_need_no_gpu():
    """every DRQ_EARG / DRQ_EWS case is decided before any launch: the pointers are made-up, aligned addresses"""
    from drqv2_amd import _lib
    lib = _lib.load()
    T, S_, D_, W = 0x10000, 0x20000, 0x30000, 0x40000
    good = dict(table=T, S=100, d=50, live=100, slots=S_, B=8, k=3, stride=1, offset=0, dist=D_, ws=W, ws_bytes=1 << 20)
    call = lambda **kw: lib.drq_explore_knn(*{**good, **kw}.values(), None)
    for bad in (dict(table=None), dict(slots=None), dict(dist=None), dict(S=0), dict(d=0), dict(d=65), dict(live=-1),
                dict(live=101), dict(B=0), dict(B=(1 << 20) + 1), dict(k=0), dict(k=9), dict(stride=0), dict(offset=-1),
                dict(offset=1), dict(stride=3, offset=3), dict(table=T + 2), dict(dist=D_ + 1), dict(slots=S_ + 4),
                dict(ws=W + 8)):
        assert call(**bad) == -1, bad
    for bad in (dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=8 * 1 * 32 - 1)):          # one chunk: G = 1
        assert call(**bad) == -2, bad
    ws = lib.drq_explore_knn_ws_bytes
    assert ws(8, 100, 1) == 8 * 1 * 32 and ws(8, 0, 1) == 0 and ws(8, 129, 1) == 8 * 2 * 32
    assert ws(256, 65536, 1) == 256 * 512 * 32 and ws(256, 1 << 20, 1) == 256 * 512 * 32          # capped at 512 per tile
    assert ws(257, 65536, 1) == 257 * 256 * 32 and ws(256, 1 << 20, 16) == 256 * 512 * 32
    assert ws(0, 100, 1) == 0 and ws(8, -1, 1) == 0 and ws(8, 100, 0) == 0


# ------------------------------------------------------------------------------------------------ the oracle
def scalar_dist(table, live, slots, k, stride, offset):
    """the contract word for word, one np.float32 scalar operation at a time"""
    out = []
    for s in slots:
        s = int(s)
        if s < 0 or s >= live:
            out.append(F(0))
            continue
        q, Ds = table[s], []
        c = offset
        while c < live:
            if c != s:
                acc = F(0)
                with np.errstate(all="ignore"):
                    for i in range(table.shape[1]):
                        t = F(q[i] - table[c][i])
                        acc = F(acc + F(t * t))
                Ds.append(F(np.inf) if np.isnan(acc) else acc)
            c += stride
        with np.errstate(all="ignore"):
            out.append(F(0) if len(Ds) < k else np.sqrt(F(sorted(Ds)[k - 1])))
    return np.array(out, F)


def same(got, want, what=None):
    assert got.dtype == want.dtype == F and got.tobytes() == want.tobytes(), (what, got, want)


@pytest.mark.parametrize("d,k", [(1, 1), (3, 2), (5, 8), (50, 3)])
def test_oracle_equals_the_scalar_loop(d, k):
    rs = np.random.RandomState(d + k)
    for live, stride, offset in ((0, 1, 0), (1, 1, 0), (k, 1, 0), (k + 1, 1, 0), (23, 1, 0), (23, 3, 0), (23, 3, 2), (23, 4, 1)):
        S = live + 3
        table = rs.standard_normal((S, d)).astype(F)
        table[live:] = np.nan
        slots = np.concatenate([rs.randint(0, max(1, live), 6), [-1, live, S - 1, 0]]).astype(np.int64)
        same(K.knn_dist(table, live, slots, k, stride, offset), scalar_dist(table, live, slots, k, stride, offset),
             (live, stride, offset))


def test_every_branch_of_the_contract_by_hand():
    t = np.array([[0.0], [3.0], [4.0], [10.0], [np.nan], [4.0]], F)          # d = 1: D = (difference)^2 exactly
    d = lambda slots, k, live=6, stride=1, offset=0: K.knn_dist(t, live, np.array(slots, np.int64), k, stride, offset).tolist()
    assert d([0], 1) == [3.0] and d([0], 2) == [4.0] and d([0], 3) == [4.0] and d([0], 4) == [10.0]
    assert d([0], 5) == [math.inf]                       # the NaN row counts as +infinity: the fifth of five others
    assert d([0], 6) == [0.0]                            # fewer than k others
    assert d([2], 1) == [0.0]                            # a duplicate elsewhere is a neighbour at distance 0 ...
    assert d([2], 1, live=5) == [1.0]                    # ... unless it lies beyond live
    assert d([-1, 6, 7], 1) == [0.0, 0.0, 0.0]           # outside the live rows
    assert d([4], 1) == [math.inf]                       # a NaN query: every D is NaN, that is +infinity
    # stride 2, offset 1: candidates 1, 3, 5.  slot 3 is on the lattice (two others), slot 0 off it (three)
    assert d([3], 2, stride=2, offset=1) == [7.0] and d([3], 3, stride=2, offset=1) == [0.0]
    assert d([0], 3, stride=2, offset=1) == [10.0] and d([0], 1, stride=2, offset=1) == [3.0]
    assert d([0], 1, live=1) == [0.0] and d([0], 1, live=0) == [0.0]
    big = np.array([[1e19, 0.0], [-1e19, 0.0], [0.0, 0.0]], F)              # D overflows to +infinity
    assert K.knn_dist(big, 3, np.array([0]), 2).tolist() == [math.inf]


@pytest.mark.parametrize("d", [3, 50, 64])
def test_the_gpu_inputs_tell_a_contracted_build_from_a_correct_one(d):
    """t * t + acc rounded once (an fma, what hipcc's default contraction would emit) against the contract's two
    roundings, on the very inputs tests/test_hip_knn.py uses: some output bit differs, so a kernel built without
    -ffp-contract=off cannot pass there.  (d = 1 has a single product and no sum to fuse.)"""
    differing = total = 0
    for k in K.KS:
        for B, live, stride, offset in K.entry_cases(d, k):
            if B != 65 or live < 65:
                continue
            table, slots = K.entry_inputs(d, B, live)
            a, b = K.knn_dist(table, live, slots, k, stride, offset), K.knn_dist_fused(table, live, slots, k, stride, offset)
            differing += int((a.view(np.uint32) != b.view(np.uint32)).sum())
            total += B
    assert differing >= 1, (differing, total)


def test_lattice_draws_and_slot_arithmetic():
    o = K.KnnOracle(R=4, N=3, dim=2, k=1, beta=0.5, candidates=5, seed=9)
    assert o.live == 0 and o.lattice() == (1, 0)
    for T in range(1, 7):
        o.observe(np.full((3, 2), T, F), T)
    assert o.live == 12 and o.rows == 6
    assert o.table[:, 0].tolist() == [5, 5, 5, 6, 6, 6, 3, 3, 3, 4, 4, 4]            # rows 5 and 6 wrapped onto 1 and 2
    rs = np.random.RandomState(9)
    rs.randint(0, 1)                                                                 # the draw of the empty table above
    for _ in range(5):
        assert o.lattice() == (3, int(rs.randint(0, 3)))                             # ceil(12 / 5) = 3
    assert K.KnnOracle(4, 3, 2, 1, 0.5).lattice() == (1, 0)


# ------------------------------------------------------------------------------------------------ the classes, no GPU
def cpu_store(R=16, N=3, **kw):
    from drqv2_amd.replay import VecFrameReplay
    return VecFrameReplay(R, N, 2, 3, 0.99, "cpu", seed=1, **kw)


def test_constructor_arguments_are_checked():
    from drqv2_amd.explore import KnnBonus, RandomFeatures
    st = cpu_store()
    for bad in (0, 65, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="dim"):
            KnnBonus(st, dim=bad)
    for bad in (0, 9, 1.0, None, False):
        with pytest.raises(ValueError, match=r"\bk must"):
            KnnBonus(st, k=bad)
    for bad in (float("nan"), float("inf"), -0.1):
        with pytest.raises(ValueError, match="beta"):
            KnnBonus(st, beta=bad)
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="candidates"):
            KnnBonus(st, candidates=bad)
    with pytest.raises(ValueError, match="seed"):
        KnnBonus(st, seed=1.5)
    with pytest.raises(ValueError, match="store"):
        KnnBonus(object())
    used = cpu_store()
    used.T = 4
    with pytest.raises(ValueError, match="before the first add"):
        KnnBonus(used)
    b = KnnBonus(st, dim=7, k=2, beta=0.25, candidates=10, seed=-1)
    assert b.table.shape == (48, 7) and b.table.dtype == torch.float32 and not b.table.any()
    assert b.seed == 0xFFFFFFFF and b.rows == 0 and b.live == 0 and b.last_dist is None
    for bad in ((9, 84), (9, 84, 85), (5, 84, 84)):
        with pytest.raises(ValueError, match="obs_shape"):
            RandomFeatures(bad, device="cpu")
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="dim"):
            RandomFeatures(dim=bad, device="cpu")
    with pytest.raises(ValueError, match="seed"):
        RandomFeatures(device="cpu", seed="0")


def test_observe_and_apply_check_before_anything_runs_and_a_cpu_device_is_refused_last():
    from drqv2_amd._lib import DrqError
    from drqv2_amd.explore import KnnBonus
    from drqv2_amd.replay import IndexedBatch
    st = cpu_store()
    b = KnnBonus(st, dim=4)
    y = torch.zeros(3, 4)
    st.T = 1                                                                  # as if add() had written row 0
    for bad, what in ((y.numpy(), "tensor"), (y[:2], "shape"), (torch.zeros(3, 5), "shape"), (y.double(), "float32")):
        with pytest.raises(ValueError, match=what):
            b.observe(bad)
    with pytest.raises(DrqError, match="GPU"):                                # well formed and aligned: only now the device
        b.observe(y)
    assert b.rows == 0 and not b.table.any()
    idx = torch.zeros((3, 5), dtype=torch.int64)
    batch = st._batch(False, idx, torch.zeros(5, 2), torch.zeros(5, 1), torch.zeros(5, 1))
    assert batch.slots.data_ptr() == idx[2].data_ptr()
    plain = IndexedBatch(st.frames, idx[0], torch.zeros(5, 2), torch.zeros(5, 1), torch.zeros(5, 1), idx[1])
    with pytest.raises(ValueError, match="indexed batch"):
        b.apply(plain)
    with pytest.raises(ValueError, match="indexed batch"):
        b.apply((idx[0], None, torch.zeros(5, 1), None, idx[1]))
    wrong = st._batch(False, idx, torch.zeros(5, 2), torch.zeros(5), torch.zeros(5, 1))
    with pytest.raises(ValueError, match="reward"):
        b.apply(wrong)
    state = b.rng.get_state()[1].copy()
    with pytest.raises(DrqError, match="GPU"):
        b.apply(batch)
    assert np.array_equal(b.rng.get_state()[1], state) and not batch[2].any()


def test_observe_refuses_a_row_twice_and_a_skipped_row():
    from drqv2_amd.explore import KnnBonus
    st = cpu_store()
    b = KnnBonus(st, dim=4)
    y = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="already"):                          # nothing added yet
        b.observe(y)
    b.rows, st.T = 5, 5
    with pytest.raises(ValueError, match="has its features already"):         # twice for row 4
        b.observe(y)
    st.T = 7
    with pytest.raises(ValueError, match=r"added 2 rows .* rows 5 \.\. 5 are missing"):
        b.observe(y)
    assert b.rows == 5


def filled(seed=3, **kw):
    from drqv2_amd.explore import KnnBonus
    b = KnnBonus(cpu_store(), dim=4, k=2, beta=0.1, candidates=7, seed=seed, **kw)
    b.rows = 19                                                               # wrapped: all 48 slots live
    b.table.copy_(torch.from_numpy(np.random.RandomState(seed).standard_normal((48, 4)).astype(F)))
    b.rng.randint(0, 5, size=3)
    return b


def test_state_dict_round_trip_and_every_rejection():
    from drqv2_amd.explore import KnnBonus
    b = filled()
    sd = b.state_dict()
    assert sd["format"] == 1 and sd["kind"] == "KnnBonus" and sd["rows"] == 19
    assert sd["config"] == {"R": 16, "N": 3, "dim": 4, "k": 2, "beta": 0.1, "candidates": 7, "seed": 3}
    assert sd["table"].shape == (48, 4) and not sd["table"].is_cuda
    part = KnnBonus(cpu_store(), dim=4)
    part.rows = 5
    assert part.state_dict()["table"].shape == (15, 4)                        # the live prefix only
    fresh = KnnBonus(cpu_store(), dim=4, k=2, beta=0.1, candidates=7, seed=3)
    fresh.table.fill_(9.0)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.table, b.table) and fresh.rows == 19 and fresh.last_dist is None
    assert [fresh.lattice() for _ in range(6)] == [b.lattice() for _ in range(6)]
    sd["table"][0, 0] = 77.0                                                  # shares nothing with either object
    assert float(b.table[0, 0]) != 77.0 and float(fresh.table[0, 0]) != 77.0
    part.load_state_dict(dict(part.state_dict()))
    fresh.table.fill_(9.0)
    sd5 = dict(sd, rows=5, table=sd["table"][:15].clone())
    fresh.load_state_dict(sd5)
    assert fresh.rows == 5 and fresh.live == 15 and not fresh.table[15:].any()          # above the live rows: zero
    for field, kw in (("dim", dict(dim=5)), ("k", dict(k=3)), ("beta", dict(beta=0.2)), ("candidates", dict(candidates=None)),
                      ("seed", dict(seed=4))):
        other = KnnBonus(cpu_store(), **{**dict(dim=4, k=2, beta=0.1, candidates=7, seed=3), **kw})
        with pytest.raises(ValueError, match=rf"\b{field}: saved"):
            other.load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bR: saved 16, here 17"):
        KnnBonus(cpu_store(R=17), dim=4, k=2, beta=0.1, candidates=7, seed=3).load_state_dict(sd)
    target = filled()
    before = target.table.clone()
    rng = sd["rng"]
    for bad in (dict(sd, kind="SimHashBonus"), dict(sd, format=2), dict(sd, rows=-1), dict(sd, rows=True), dict(sd, rows=3),
                dict(sd, table=sd["table"].double()), dict(sd, table=sd["table"][:, :3]), dict(sd, rng=None),
                dict(sd, rng=(rng[0], rng[1][:10], rng[2], rng[3], rng[4])), {k: v for k, v in sd.items() if k != "table"},
                {k: v for k, v in sd.items() if k != "config"}, None):
        with pytest.raises(ValueError):
            target.load_state_dict(bad)
        assert torch.equal(target.table, before) and target.rows == 19


def test_checkpoint_file_round_trip(tmp_path):
    from drqv2_amd import checkpoint
    from drqv2_amd.explore import KnnBonus, RandomFeatures
    b = filled()
    path, without = str(tmp_path / "knn.pt"), str(tmp_path / "plain.pt")
    checkpoint.save(path, bonus=b, extra={"step": 19})
    checkpoint.save(without, extra={"step": 1})
    fresh = KnnBonus(cpu_store(), dim=4, k=2, beta=0.1, candidates=7, seed=3)
    assert checkpoint.load(path, bonus=fresh) == {"step": 19}
    assert torch.equal(fresh.table, b.table) and fresh.rows == 19
    assert [fresh.lattice() for _ in range(4)] == [b.lattice() for _ in range(4)]
    with pytest.raises(ValueError, match="bonus"):
        checkpoint.load(without, bonus=fresh)
    with pytest.raises(ValueError, match=r"\bk: saved 2, here 3"):
        checkpoint.load(path, bonus=KnnBonus(cpu_store(), dim=4, k=3, beta=0.1, candidates=7, seed=3))
    f = RandomFeatures(dim=6, device="cpu", seed=5)
    assert f.state_dict() == {"format": 1, "kind": "RandomFeatures", "config": {"obs_shape": (9, 84, 84), "dim": 6, "seed": 5}}
    f.load_state_dict(f.state_dict())
    with pytest.raises(ValueError, match=r"\bseed: saved 5, here 6"):
        RandomFeatures(dim=6, device="cpu", seed=6).load_state_dict(f.state_dict())


def test_random_features_on_the_cpu_are_a_function_of_the_seed_and_move_no_generator():
    from drqv2_amd._lib import DrqError
    from drqv2_amd.explore import RandomFeatures
    torch.manual_seed(123)
    before = torch.get_rng_state()
    a, b, c = (RandomFeatures(dim=6, device="cpu", seed=s) for s in (5, 5, 6))
    assert torch.equal(torch.get_rng_state(), before)
    wa, wb, wc = (torch.cat([p.reshape(-1).double() for m in (f.encoder, f.head) for p in m.parameters()]) for f in (a, b, c))
    assert torch.equal(wa, wb) and not torch.equal(wa, wc)
    assert not any(p.requires_grad for m in (a.encoder, a.head) for p in m.parameters())
    obs = torch.zeros((2, 9, 84, 84), dtype=torch.uint8)
    for bad, what in ((obs.numpy(), "tensor"), (obs[:, :3], "shape"), (obs.float(), "uint8"), (obs[0], "shape")):
        with pytest.raises(ValueError, match=what):
            a(bad)
    with pytest.raises(DrqError, match="GPU"):
        a(obs)
