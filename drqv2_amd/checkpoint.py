"""Checkpoint and resume for the vectorised training loop (new; the reference pickles its agent and keeps its replay as
episode files, train.py:192-204 -- the step-major stores, the device environment and the episode statistics live in HBM
and nothing else held what is in them).

The contract: a run that is saved, torn down and restored continues exactly as the uninterrupted run would have, bit for
bit -- actions, batches, priorities, weights, statistics and environment state.  Everything in the loop is deterministic
for a seed, so the state is all there is to keep:

  agent      DrQV2Agent.__getstate__(): weights, target network, Adam moments and step counts (no second format)
  store      VecDeviceReplay / VecFrameReplay.state_dict(): T, the live slots of the ring, the store's RandomState, the
             priority tree and priority_beta
  iterator   BatchIterator.state_dict(): the one batch of look-ahead, which was drawn BEFORE the save and has consumed its
             random numbers
  env        VecReach / VecPointMass.state_dict(): the task, action_repeat and the state words of every environment (seven;
             nine with the point mass's velocity); the frames are drawn again from them
  stats      VecEpisodeStats.state_dict(): the running returns and lengths, the totals and the log
  bonus      SimHashBonus.state_dict() (optional, `bonus=`): the count table of the exploration bonus in sparse form; or
             KnnBonus.state_dict(): the live rows of its feature table, the row counter and its RandomState
  rng        torch.get_rng_state() and torch.cuda.get_rng_state(device): update()'s draws and act_batch()'s noise

        for step in range(start, steps):
            ...                                             # act_batch, env.step, store.add, stats.step, agent.update
            if (step + 1) % every == 0:
                checkpoint.save(path, agent=agent, store=store, iterator=it, env=env, stats=stats, extra={"step": step + 1})
        ...
        extra = checkpoint.load(path, agent=agent, store=store, iterator=it, env=env, stats=stats)      # on fresh objects

save() synchronises the device (every state_dict() does) and takes the ring through host memory whole: 21,168 bytes per
live slot of a VecFrameReplay, 63,504 of a VecDeviceReplay of stacks.  Chunked or incremental ring files are out of scope.
"""
import os

import torch

FORMAT = 1


def check_state(obj, sd, config=None, tensors=None, kind=None):
    """What every load_state_dict() does before it changes anything: `sd` is a dict of this format and of obj's kind,
    its "config" equals `config` (obj's own) field for field, and every tensor it holds for a name in `tensors` (name ->
    the tensor of obj it goes into, or a (shape, dtype) pair) has that shape and dtype.  ValueError naming EVERY field
    that differs; nothing has been touched then."""
    kind = kind or type(obj).__name__
    if not isinstance(sd, dict):
        raise ValueError(f"{kind}.load_state_dict(): a dict from state_dict() required, got {type(sd).__name__}")
    if sd.get("format") != FORMAT or sd.get("kind") != kind:
        raise ValueError(f"{kind}.load_state_dict(): format {FORMAT} of kind {kind!r} required, got format "
                         f"{sd.get('format')!r} of kind {sd.get('kind')!r}")
    bad = []
    if config is not None:
        saved = sd.get("config")
        if not isinstance(saved, dict):
            raise ValueError(f"{kind}.load_state_dict(): the state holds no configuration")
        for k, mine in config.items():
            theirs = saved.get(k, "<absent>")
            if isinstance(theirs, list):
                theirs = tuple(theirs)
            if theirs != mine:
                bad.append(f"{k}: saved {theirs!r}, here {mine!r}")
    for name, want in (tensors or {}).items():
        shape, dtype = (tuple(want.shape), want.dtype) if torch.is_tensor(want) else want
        t = sd.get(name)
        if not torch.is_tensor(t):
            bad.append(f"{name}: no tensor saved")
        elif tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            bad.append(f"{name}: saved {t.dtype} {tuple(t.shape)}, here {dtype} {tuple(shape)}")
    if bad:
        raise ValueError(f"{kind}.load_state_dict(): the saved state does not fit this object -- " + "; ".join(bad))


def host(t):
    """a copy of tensor t in host memory that shares nothing with it"""
    return t.detach().to("cpu", copy=True)


def _device(*objs):
    """the GPU whose generator the loop draws from: that of the first object given that lives on one, or None"""
    for o in objs:
        d = getattr(o, "device", None)
        if d is None:
            continue
        d = torch.device(d)
        if d.type == "cuda":
            return torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index)
    return None


def save(path, *, agent=None, store=None, iterator=None, env=None, stats=None, bonus=None, extra=None):
    """Writes one file that holds the state of every object given (module docstring) and `extra` -- plain data of the
    caller's: numbers, strings, lists, dicts, tensors -- which load() hands back.  bonus= is the SimHashBonus of a loop that
    has one (drqv2_amd/explore.py); a file saved without it is what it always was.  The generator states are torch's
    default CPU generator and the default generator of the agent's (else the store's, environment's, statistics') GPU.
    SYNCHRONISES that device.  Atomic: the file is written to path + ".tmp", flushed and fsynced, then renamed onto
    path, so a process killed during a save leaves the previous checkpoint intact."""
    path = os.fspath(path)
    ck = {"format": FORMAT, "kind": "checkpoint", "extra": extra}
    if agent is not None:
        ck["agent"] = agent.__getstate__()
    for name, obj in (("store", store), ("iterator", iterator), ("env", env), ("stats", stats), ("bonus", bonus)):
        if obj is not None:
            ck[name] = obj.state_dict()
    dev = _device(agent, store, env, stats, bonus)
    ck["rng"] = {"cpu": torch.get_rng_state(),
                 "cuda": torch.cuda.get_rng_state(dev) if dev is not None and torch.cuda.is_available() else None}
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(ck, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def _check_agent(agent, st):
    """the constructor arguments of the saved agent against this one's (the device aside): ValueError naming every one
    that differs"""
    if not isinstance(st, dict) or "init" not in st:
        raise ValueError("checkpoint.load(): the file's agent is no DrQV2Agent.__getstate__() snapshot")
    mine, saved = agent._init_kwargs, st["init"]
    norm = lambda v: tuple(v) if isinstance(v, (list, tuple)) else v
    bad = [f"{k}: saved {saved.get(k)!r}, here {v!r}" for k, v in mine.items()
           if k != "device" and norm(saved.get(k, "<absent>")) != norm(v)]
    if bad:
        raise ValueError("checkpoint.load(): the saved agent does not fit this one -- " + "; ".join(bad))


def load(path, *, agent=None, store=None, iterator=None, env=None, stats=None, bonus=None):
    """Restores, from a file save() wrote, every object given -- freshly constructed or used -- and returns `extra`.
    The agent is loaded IN PLACE by the logic of DrQV2Agent.__setstate__ (its constructor arguments must equal the saved
    ones, the device aside); the store before its iterator, whose look-ahead batch is rebuilt over the restored ring; the
    exploration bonus's count table (bonus=) when asked for; the generator states last, so nothing the restore itself draws or launches moves them.  A part that is in the file but
    not asked for is ignored.  ValueError, before anything is changed: a part that is asked for but not in the file, a
    file that is no checkpoint of this format.  Each part then checks its configuration before it changes itself
    (ValueError naming every field that differs)."""
    ck = torch.load(os.fspath(path), map_location="cpu", weights_only=True)     # plain data only: no code is unpickled
    if not isinstance(ck, dict) or ck.get("format") != FORMAT or ck.get("kind") != "checkpoint":
        raise ValueError(f"checkpoint.load(): {path} is no checkpoint of format {FORMAT}")
    asked = [(n, o) for n, o in (("agent", agent), ("store", store), ("iterator", iterator), ("env", env), ("stats", stats),
                                 ("bonus", bonus)) if o is not None]
    missing = [n for n, _ in asked if n not in ck]
    if missing:
        raise ValueError(f"checkpoint.load(): {path} holds no {', '.join(missing)} (it holds "
                         f"{', '.join(n for n in ('agent', 'store', 'iterator', 'env', 'stats', 'bonus') if n in ck) or 'none'})")
    if agent is not None:
        _check_agent(agent, ck["agent"])
    for name, obj in asked:
        if name == "agent":
            obj._restore(ck["agent"])
        else:
            obj.load_state_dict(ck[name])
    rng = ck.get("rng") or {}
    if rng.get("cpu") is not None:
        torch.set_rng_state(rng["cpu"])
    dev = _device(agent, store, env, stats, bonus)
    if rng.get("cuda") is not None and dev is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(rng["cuda"], dev)
    return ck.get("extra")
