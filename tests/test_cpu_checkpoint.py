"""Checkpoint and resume (drqv2_amd/checkpoint.py; state_dict() / load_state_dict() of the step-major stores, their
iterator, the episode statistics and the device environment): everything that needs no GPU.  A CPU store holds its ring
in host tensors and no launch is involved in saving or loading it, so the round trip is complete here; the environment's
load ends in a launch and is refused on the CPU after its checks.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib, checkpoint
from drqv2_amd.envs import VecReach
from drqv2_amd.replay import BatchIterator, DeviceReplay, VecDeviceReplay, VecEpisodeStats, VecFrameReplay
from tests import abi

R, N, A = 12, 3, 2
RING = ("frames", "action", "reward", "discount", "first")


def make(cls, seed, rows=R, n=N, a=A, nstep=3, discount=0.99, guard_rows=2, indexed=True):
    if cls is VecFrameReplay:
        return cls(rows, n, a, nstep, discount, "cpu", seed=seed, guard_rows=guard_rows, indexed=indexed)
    return cls(rows, n, (3, 8, 8), a, nstep, discount, "cpu", seed=seed, guard_rows=guard_rows, indexed=indexed)


def fill(store, T, seed):
    """T, the arrays and the generator written by hand: every slot of the ring gets random bytes, the generator is moved"""
    g = torch.Generator().manual_seed(seed)
    store.frames.copy_(torch.randint(0, 256, store.frames.shape, generator=g, dtype=torch.uint8))
    store.action.copy_(torch.rand(store.action.shape, generator=g))
    store.reward.copy_(torch.rand(store.reward.shape, generator=g))
    store.discount.copy_(torch.rand(store.discount.shape, generator=g))
    store.first.copy_(torch.randint(0, 2, store.first.shape, generator=g, dtype=torch.uint8))
    store.T = T
    store.priority_beta = 0.7
    store.rng.random_sample(seed)
    return store


def arrays(store):
    return {n: getattr(store, n).clone() for n in RING}


# ------------------------------------------------------------------------------------------------ the stores
@pytest.mark.parametrize("cls", [VecDeviceReplay, VecFrameReplay])
@pytest.mark.parametrize("T", [5, R, 31])
def test_store_round_trip_on_the_cpu(cls, T):
    """state_dict() -> load_state_dict() into a second store with another seed: equal live slots, T, priority_beta and
    an equal next random_sample((4, 4)); T < R saves T N slots and the slots above them are the constructor's"""
    src = fill(make(cls, 1), T, 7)
    sd = src.state_dict()
    live = min(T, R) * N
    assert sd["format"] == 1 and sd["kind"] == cls.__name__ and sd["T"] == T
    for n in RING:
        assert not sd[n].is_cuda and sd[n].shape[0] == live, n
        assert sd[n].data_ptr() != getattr(src, n).data_ptr()              # a copy: the store may go on
    dst = fill(make(cls, 2), 9, 3)
    dst.last_steps = dst.last_index = "stale"
    dst.load_state_dict(sd)
    assert dst.T == T and dst.priority_beta == 0.7 and dst.last_steps is None and dst.last_index is None
    for n in RING:
        assert torch.equal(getattr(dst, n)[:live], getattr(src, n)[:live]), n
    fresh = make(cls, 0)
    for n in RING[1:]:                                                     # frames above the live slots are torch.empty
        assert torch.equal(getattr(dst, n)[live:], getattr(fresh, n)[live:]), n
    assert np.array_equal(dst.rng.random_sample((4, 4)), src.rng.random_sample((4, 4)))
    assert dst.bounds() == src.bounds() and len(dst) == len(src)


def test_store_round_trip_through_a_file(tmp_path):
    src, stats = fill(make(VecFrameReplay, 1), 31, 7), VecEpisodeStats(N, "cpu", log_size=8, max_episodes_per_env=2)
    stats.episode_return.copy_(torch.tensor([1.5, 2.5, 3.5]))
    stats.header[1] = 4
    stats._log[3][2] = 99
    stats.rows = 17
    path = str(tmp_path / "ck.pt")
    torch.manual_seed(3)
    checkpoint.save(path, store=src, iterator=iter(src), stats=stats, extra={"step": 31, "note": "x"})
    want = torch.rand(4)
    dst, stats2 = make(VecFrameReplay, 5), VecEpisodeStats(N, "cpu", log_size=8, max_episodes_per_env=2)
    it = iter(dst)
    torch.manual_seed(99)
    assert checkpoint.load(path, store=dst, iterator=it, stats=stats2) == {"step": 31, "note": "x"}
    assert torch.equal(torch.rand(4), want)                                # the generator state is restored, last
    for n in RING:
        assert torch.equal(getattr(dst, n), getattr(src, n)), n
    assert stats2.rows == 17 and torch.equal(stats2.episode_return, stats.episode_return)
    assert torch.equal(stats2.header, stats.header) and all(torch.equal(a, b) for a, b in zip(stats2._log, stats._log))
    assert it._ahead is None
    assert checkpoint.load(path, store=make(VecFrameReplay, 6)) == {"step": 31, "note": "x"}     # other parts are ignored


MISMATCH = [("R", dict(rows=13)), ("N", dict(n=4)), ("A", dict(a=3)), ("nstep", dict(nstep=2)), ("gamma", dict(discount=0.9)),
            ("guard_rows", dict(guard_rows=3)), ("indexed", dict(indexed=False))]


@pytest.mark.parametrize("field,kw", MISMATCH)
def test_every_configuration_mismatch_is_named_and_nothing_changes(field, kw):
    sd = fill(make(VecFrameReplay, 1), 31, 7).state_dict()
    dst = fill(make(VecFrameReplay, 2, **kw), 9, 3)
    before, rng = arrays(dst), dst.rng.get_state()
    with pytest.raises(ValueError, match=rf"\b{field}: saved"):
        dst.load_state_dict(sd)
    assert dst.T == 9 and dst.priority_beta == 0.7
    assert all(torch.equal(getattr(dst, n), before[n]) for n in RING)
    assert all(np.array_equal(a, b) for a, b in zip(rng, dst.rng.get_state()))


def test_every_differing_field_is_named_at_once_and_the_rest_of_the_configuration():
    sd = fill(make(VecFrameReplay, 1), 31, 7).state_dict()
    with pytest.raises(ValueError) as e:
        make(VecFrameReplay, 2, rows=13, a=3, nstep=2).load_state_dict(sd)
    assert all(f"{k}: saved" in str(e.value) for k in ("R", "A", "nstep"))
    for k, v in (("slot_shape", (3, 8, 8)), ("priority_alpha", 0.6), ("priority_eps", 1e-3)):
        bad = dict(sd, config=dict(sd["config"], **{k: v}))                # fields a CPU store cannot be built to differ in
        with pytest.raises(ValueError, match=rf"\b{k}: saved"):
            make(VecFrameReplay, 2).load_state_dict(bad)
    with pytest.raises(ValueError, match="kind"):                          # the class is part of the configuration
        make(VecDeviceReplay, 2).load_state_dict(sd)


def test_wrong_format_kind_shapes_and_frames_false():
    src = fill(make(VecFrameReplay, 1), 31, 7)
    sd = src.state_dict()
    dst = fill(make(VecFrameReplay, 2), 9, 3)
    before = arrays(dst)
    for bad in (dict(sd, format=2), dict(sd, kind="VecReach"), {k: v for k, v in sd.items() if k != "format"}, None,
                dict(sd, T=-1), dict(sd, T=5), dict(sd, reward=sd["reward"][:-1]), dict(sd, first=sd["first"].float()),
                {k: v for k, v in sd.items() if k != "rng"}):
        with pytest.raises(ValueError):
            dst.load_state_dict(bad)
    light = src.state_dict(frames=False)
    assert not any(n in light for n in RING) and light["T"] == 31
    with pytest.raises(ValueError, match="frames=False"):
        dst.load_state_dict(light)
    assert dst.T == 9 and all(torch.equal(getattr(dst, n), before[n]) for n in RING)
    dst.load_state_dict(light, frames=False)                               # the caller means it: the ring stays
    assert dst.T == 31 and all(torch.equal(getattr(dst, n), before[n]) for n in RING)
    assert np.array_equal(dst.rng.random_sample(5), src.rng.random_sample(5))


# ------------------------------------------------------------------------------------------------ the iterator
def test_iterator_without_a_store_and_with_nothing_pending():
    with pytest.raises(_lib.DrqError, match="store"):
        BatchIterator(lambda: None).state_dict()
    episodic = DeviceReplay(64, (9, 84, 84), A, 3, 0.99, "cpu", seed=0)
    with pytest.raises(_lib.DrqError, match="store"):
        iter(episodic).state_dict()
    store = make(VecFrameReplay, 1)
    it = iter(store)
    assert isinstance(it, BatchIterator) and it._store is store
    sd = it.state_dict()
    assert sd == {"format": 1, "kind": "BatchIterator", "pending": False}
    other = iter(make(VecFrameReplay, 2))
    other._ahead, other._drawn = "stale", "stale"
    other.load_state_dict(sd)
    assert other._ahead is None and other.state_dict() == sd
    for bad in (dict(sd, format=0), dict(sd, kind="VecFrameReplay"), []):
        with pytest.raises(ValueError):
            other.load_state_dict(bad)


def test_iterator_pending_batch_is_rebuilt_over_the_restored_ring():
    """a pending uniform batch written by hand (no draw on the CPU): it comes back as the store's own batch type, over the
    store's own frames and flags, and is handed out by the next next()"""
    from drqv2_amd.replay import FrameBatch, IndexedBatch
    for cls, kind in ((VecFrameReplay, FrameBatch), (VecDeviceReplay, IndexedBatch)):
        src = fill(make(cls, 1), 31, 7)
        B = 4
        idx = torch.arange(3 * B, dtype=torch.int64).view(3, B)
        act, rew, disc = torch.rand(B, A), torch.rand(B, 1), torch.rand(B, 1)
        steps = torch.tensor([3, 2, 0, 1], dtype=torch.int32)
        it = iter(src)
        it._ahead, it._drawn = src._batch(False, idx, act, rew, disc), (idx, steps)
        sd = it.state_dict()
        assert sd["pending"] and not sd["prioritized"] and "weights" not in sd
        dst = make(cls, 2)
        dst.load_state_dict(src.state_dict())
        it2 = iter(dst)
        it2.load_state_dict(sd)
        assert torch.equal(dst.last_index, idx) and torch.equal(dst.last_steps, steps)
        b = next(it2)
        assert type(b) is kind and b.frames is dst.frames and it2._ahead is None
        assert torch.equal(b[0], idx[0]) and torch.equal(b[4], idx[1])
        assert torch.equal(b[1], act) and torch.equal(b[2], rew) and torch.equal(b[3], disc)
        if kind is FrameBatch:
            assert b.ring[0] is dst.first and b.ring[1:] == (R, N)
        for bad in (dict(sd, action=torch.rand(B, A + 1)), dict(sd, index=idx + R * N), dict(sd, prioritized=True)):
            with pytest.raises(ValueError):
                it2.load_state_dict(bad)
        assert it2._ahead is None
    loose = make(VecFrameReplay, 1, indexed=False)
    it = iter(loose)
    it._ahead = "a materialised batch"
    with pytest.raises(_lib.DrqError, match="indexed"):
        it.state_dict()


# ------------------------------------------------------------------------------------------------ statistics, environment
def test_stats_and_env_checks_on_the_cpu():
    stats = VecEpisodeStats(N, "cpu", log_size=8, max_episodes_per_env=2)
    sd = stats.state_dict()
    assert sd["format"] == 1 and sd["kind"] == "VecEpisodeStats" and sd["rows"] == 0
    for field, kw in (("N", dict(num_envs=4)), ("W", dict(log_size=9)), ("limit", dict(max_episodes_per_env=0))):
        args = dict(num_envs=N, log_size=8, max_episodes_per_env=2)
        args.update(kw)
        other = VecEpisodeStats(device="cpu", **args)
        other.rows = 5
        with pytest.raises(ValueError, match=rf"\b{field}: saved"):
            other.load_state_dict(sd)
        assert other.rows == 5
    with pytest.raises(ValueError):
        stats.load_state_dict(dict(sd, kind="VecReach"))

    env = VecReach(N, "cpu", action_dim=A, episode_length=5, seed=3)
    sd = env.state_dict()
    assert sd["format"] == 1 and sd["kind"] == "VecReach" and set(("pos", "target", "t", "episode", "over")) <= set(sd)
    assert "frame" not in sd                                               # derived data is not state
    for field, kw in (("N", dict(num_envs=4)), ("A", dict(action_dim=3)), ("episode_length", dict(episode_length=6)),
                      ("seed", dict(seed=4))):
        args = dict(num_envs=N, action_dim=A, episode_length=5, seed=3)
        args.update(kw)
        with pytest.raises(ValueError, match=rf"\b{field}: saved"):
            VecReach(device="cpu", **args).load_state_dict(sd)
    with pytest.raises(ValueError):
        env.load_state_dict(dict(sd, format=3))
    with pytest.raises(_lib.DrqError, match="GPU"):                        # after the checks, like reset()
        env.load_state_dict(sd)
    with pytest.raises(_lib.DrqError, match="GPU"):
        env.render()


# ------------------------------------------------------------------------------------------------ the file
def test_save_is_atomic(tmp_path, monkeypatch):
    """a save that dies at the rename leaves the previous checkpoint byte for byte, and no temporary file"""
    path = str(tmp_path / "ck.pt")
    store = fill(make(VecFrameReplay, 1), 5, 7)
    checkpoint.save(path, store=store, extra={"step": 5})
    with open(path, "rb") as f:
        before = f.read()
    fill(store, 31, 8)

    def boom(*a, **k):
        raise OSError("killed")
    monkeypatch.setattr(os, "replace", boom)
    with pytest.raises(OSError, match="killed"):
        checkpoint.save(path, store=store, extra={"step": 31})
    monkeypatch.undo()
    with open(path, "rb") as f:
        assert f.read() == before
    assert os.listdir(str(tmp_path)) == ["ck.pt"]
    assert checkpoint.load(path, store=make(VecFrameReplay, 2)) == {"step": 5}


def test_load_of_an_absent_part_and_of_no_checkpoint(tmp_path):
    path = str(tmp_path / "ck.pt")
    store = fill(make(VecFrameReplay, 1), 5, 7)
    checkpoint.save(path, store=store)
    dst = fill(make(VecFrameReplay, 2), 9, 3)
    with pytest.raises(ValueError, match="stats"):
        checkpoint.load(path, store=dst, stats=VecEpisodeStats(N, "cpu"))
    assert dst.T == 9                                                      # refused before anything was restored
    with pytest.raises(ValueError, match="iterator"):
        checkpoint.load(path, iterator=iter(dst))
    torch.save({"format": 1, "kind": "something else"}, path)
    with pytest.raises(ValueError, match="no checkpoint"):
        checkpoint.load(path, store=dst)


def test_agent_goes_in_through_its_snapshot_and_loads_in_place(tmp_path):
    import drqv2
    mk = lambda seed, hidden=64: (torch.manual_seed(seed), drqv2.DrQV2Agent((9, 84, 84), (A,), "cpu", 1e-3, 20, hidden, 0.01, 8,
                                                                            1, "0.5", 0.3, True))[1]
    src = mk(1)
    src.critic_opt.t = 7
    with torch.no_grad():
        src._engine.adam_m.uniform_(-1, 1)
    path = str(tmp_path / "ck.pt")
    checkpoint.save(path, agent=src)
    dst = mk(2)
    engine, arena = dst._engine, dst._engine.params.data_ptr()
    dst.metrics_on_device = True
    checkpoint.load(path, agent=dst)
    assert dst._engine is engine and dst._engine.params.data_ptr() == arena and dst.metrics_on_device    # in place
    assert torch.equal(dst._engine.params, src._engine.params)
    for lo, hi in (src._engine.layout["seg"][net] for net in ("enc", "critic", "actor")):     # the target has no moments
        assert torch.equal(dst._engine.adam_m[lo:hi], src._engine.adam_m[lo:hi])
    assert dst.critic_opt.t == 7
    with pytest.raises(ValueError, match="hidden_dim: saved 64, here 32"):
        checkpoint.load(path, agent=mk(3, hidden=32))
    st = src.__getstate__()
    assert st["compute_dtype"] == "fp32"
    del st["compute_dtype"]                                                # a snapshot written before the key existed
    old = drqv2.DrQV2Agent.__new__(drqv2.DrQV2Agent)
    old.__setstate__(st)
    assert old._engine.bf16 is False and torch.equal(old._engine.params, src._engine.params)


# ------------------------------------------------------------------------------------------------ the interface
def test_render_entry_in_header_prototypes_and_build_rule():
    name = "drq_vec_reach_render"
    abi.assert_prototype(name)
    from drqv2_amd import build
    assert "vecenv.hip" in build.SOURCES and build.FILE_FLAGS["vecenv.hip"] == ["-ffp-contract=off"]
    lib = _lib.load()
    assert hasattr(lib, name)
    # argument errors are reported before any launch, so they need no GPU: null pointers, N, alignment
    assert lib.drq_vec_reach_render(None, None, 1, None, None) == -1
    assert lib.drq_vec_reach_render(4096, 4096, 0, 4096, None) == -1
    assert lib.drq_vec_reach_render(4096, 4096, 1 << 31, 4096, None) == -1
    assert lib.drq_vec_reach_render(4096, 4096, 1, 4096 + 8, None) == -1
    assert lib.drq_vec_reach_render(4096 + 2, 4096, 1, 4096, None) == -1
    for method in ("render", "state_dict", "load_state_dict"):
        assert callable(getattr(VecReach, method))
