"""CPU-only checks of the drop-in boundary: constructor/method signatures and state_dict layout against
fixtures captured from the reference (tests/golden/interface.json), the C ABI export table against
include/drqv2_hip.h, the config surface, pickling, and the loud failure of the update path without a GPU."""
import inspect
import json
import os
import pickle
import re

import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def iface():
    with open(os.path.join(G, "interface.json")) as f:
        return json.load(f)


def _sig(f):
    return [[n, None if p.default is inspect._empty else repr(p.default)]
            for n, p in inspect.signature(f).parameters.items()]


def test_signatures_match_reference(iface):
    import drqv2
    import utils
    objs = {"DrQV2Agent.__init__": drqv2.DrQV2Agent.__init__, "DrQV2Agent.act": drqv2.DrQV2Agent.act,
            "DrQV2Agent.update": drqv2.DrQV2Agent.update, "DrQV2Agent.train": drqv2.DrQV2Agent.train,
            "DrQV2Agent.update_critic": drqv2.DrQV2Agent.update_critic,
            "DrQV2Agent.update_actor": drqv2.DrQV2Agent.update_actor,
            "RandomShiftsAug.__init__": drqv2.RandomShiftsAug.__init__, "Encoder.__init__": drqv2.Encoder.__init__,
            "Actor.__init__": drqv2.Actor.__init__, "Actor.forward": drqv2.Actor.forward,
            "Critic.__init__": drqv2.Critic.__init__, "Critic.forward": drqv2.Critic.forward,
            "utils.soft_update_params": utils.soft_update_params, "utils.to_torch": utils.to_torch,
            "utils.schedule": utils.schedule, "utils.weight_init": utils.weight_init,
            "utils.TruncatedNormal.__init__": utils.TruncatedNormal.__init__,
            "utils.TruncatedNormal.sample": utils.TruncatedNormal.sample,
            "utils.set_seed_everywhere": utils.set_seed_everywhere, "utils.Until.__init__": utils.Until.__init__,
            "utils.Every.__init__": utils.Every.__init__}
    for name, fn in objs.items():
        assert _sig(fn) == iface["signatures"][name], name
    for n in iface["utils_names"]:          # every public name train.py can reach
        assert hasattr(utils, n), n


def test_state_dict_init_stream_and_attrs(iface):
    import drqv2
    torch.manual_seed(1)
    ag = drqv2.DrQV2Agent((9, 84, 84), (6,), "cpu", 1e-4, 50, 1024, 0.01, 2000, 2, "linear(1.0,0.1,500000)", 0.3, True)
    for nm in ("encoder", "actor", "critic", "critic_target"):
        got = [[k, list(v.shape)] for k, v in getattr(ag, nm).state_dict().items()]
        assert got == iface["state_dict"][nm], nm
    # same global-RNG consumption as the reference constructors -> same initial weights under seed 1
    for nm in ("encoder", "actor", "critic"):
        for p, r in zip(getattr(ag, nm).parameters(), iface["init_seed1"][nm]):
            assert float(p.detach().double().norm()) == pytest.approx(r["l2"], rel=1e-9, abs=1e-12), nm
    for a, b in zip(ag.critic.parameters(), ag.critic_target.parameters()):
        assert torch.equal(a, b)
    assert ag.encoder.repr_dim == iface["repr_dim"]
    for attr in iface["agent_attrs"]:
        assert hasattr(ag, attr), attr
    assert ag.training is True
    ag.train(False)
    assert ag.training is False and not ag.encoder.training
    # parameters live in one arena, gradients are views of the gradient arena
    eng = ag._engine
    p0 = next(ag.critic.parameters())
    assert p0.data_ptr() == eng.params.data_ptr() + 4 * eng.layout["critic"][0]
    assert p0.grad.data_ptr() == eng.grads.data_ptr() + 4 * eng.layout["critic"][0]


def test_update_and_act_fail_loudly_without_gpu():
    import drqv2
    from drqv2_amd._lib import DrqError
    from drqv2_amd import synth
    ag = drqv2.DrQV2Agent((9, 84, 84), (3,), "cpu", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, True)
    assert ag.update(iter([]), 1) == {}          # gated step: no batch is drawn (drqv2.py:233-234)
    batch = synth.make_batch(2, 3)
    with pytest.raises(DrqError):
        ag.update(iter([tuple(x.numpy() for x in batch)]), 0)
    with pytest.raises(DrqError):
        ag.act(batch[0][0].numpy(), 0, True)
    import utils
    with pytest.raises(DrqError):
        utils.soft_update_params(torch.nn.Linear(4, 4), torch.nn.Linear(4, 4), 0.01)


def test_pickle_roundtrip_cpu():
    import drqv2
    ag = drqv2.DrQV2Agent((9, 84, 84), (3,), "cpu", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, False)
    ag.critic_opt.t = 7
    with torch.no_grad():
        ag._engine.adam_m.uniform_(-1, 1)
    state = torch.get_rng_state()
    ag2 = pickle.loads(pickle.dumps(ag))
    assert torch.equal(torch.get_rng_state(), state)             # loading must not move the global RNG
    for a, b in zip(ag.actor.parameters(), ag2.actor.parameters()):
        assert torch.equal(a, b)
    seg = ag._engine.layout["seg"]["critic"]
    assert ag2.critic_opt.t == 7
    assert torch.equal(ag2._engine.adam_m[seg[0]:seg[1]], ag._engine.adam_m[seg[0]:seg[1]])
    assert ag2.use_tb is False and ag2.stddev_schedule == "0.2"


def test_reference_format_snapshot_loads():
    """A snapshot written by the reference (train.py:192-198) is a pickle of ITS agent object: class path
    `drqv2.DrQV2Agent`, state = the object's __dict__ (modules, torch.optim.Adam objects, scalars).  With this
    repo's drqv2.py on the path pickle hands that dict to DrQV2Agent.__setstate__; the stand-in below produces
    exactly such a pickle stream (the reference itself cannot be imported in the test suite)."""
    import drqv2
    torch.manual_seed(3)
    src = drqv2.DrQV2Agent((9, 84, 84), (3,), "cpu", 2e-4, 20, 64, 0.02, 1500, 2, "linear(1.0,0.1,1000)", 0.25, False)
    mods = {n: getattr(src, n) for n in ("encoder", "actor", "critic", "critic_target")}
    ref_state = dict(device="cpu", critic_target_tau=0.02, update_every_steps=2, use_tb=False, num_expl_steps=1500,
                     stddev_schedule="linear(1.0,0.1,1000)", stddev_clip=0.25, training=True, aug=None, **mods)
    for n, m in (("encoder_opt", src.encoder), ("actor_opt", src.actor), ("critic_opt", src.critic)):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
        opt = torch.optim.Adam(ps, lr=2e-4)
        for k in range(3):                                   # three real Adam steps populate exp_avg / exp_avg_sq / step
            for p in ps:
                p.grad = torch.randn_like(p) * 0.1
            opt.step()
        ref_state[n] = opt

    class RefPickle:                                         # pickles as the reference's object would:
        def __reduce__(self):                                # new object of class drqv2.DrQV2Agent, then setstate
            return (object.__new__, (drqv2.DrQV2Agent,), ref_state)

    ag = pickle.loads(pickle.dumps(RefPickle()))
    assert isinstance(ag, drqv2.DrQV2Agent) and ag.critic_target_tau == 0.02 and ag.stddev_clip == 0.25
    assert ag.num_expl_steps == 1500 and ag.use_tb is False and ag.actor_opt.lr == 2e-4
    for n, m in mods.items():
        for (k, a), (_, b) in zip(m.state_dict().items(), getattr(ag, n).state_dict().items()):
            assert torch.equal(a.detach().cpu(), b.detach().cpu()), (n, k)
    eng = ag._engine
    for net, on in (("enc", "encoder_opt"), ("actor", "actor_opt"), ("critic", "critic_opt")):
        ref = ref_state[on].state_dict()["state"]
        assert getattr(ag, on).t == 3
        for i, off in enumerate(eng.layout[net]):
            m = ref[i]["exp_avg"].reshape(-1)
            assert torch.equal(eng.adam_m[off:off + m.numel()].cpu(), m)
            assert torch.equal(eng.adam_v[off:off + m.numel()].cpu(), ref[i]["exp_avg_sq"].reshape(-1))


def test_state_written_by_the_reference_loads_and_round_trips():
    """tests/golden/ref_state.pt was written by the REFERENCE's own agent (make_golden.py gen_ref_state: two of its
    updates, then module / torch.optim.Adam state_dicts as plain tensors).  It loads with weights_only=True, goes
    into this agent's arenas, and export_reference_state() gives the same tensors back; make_golden.py also checked,
    where the reference runs, that the reference's objects load that export and keep training."""
    import drqv2
    st = torch.load(os.path.join(ROOT, "tests", "golden", "ref_state.pt"), weights_only=True)
    d = st["dims"]
    ag = drqv2.DrQV2Agent((d["C"], 84, 84), (d["A"],), "cpu", 5e-4, d["F"], d["H"], 0.01, 2000, 2, "0.2", 0.3, True)
    ag.import_reference_state(st)
    eng = ag._engine
    assert (ag.encoder_opt.t, ag.actor_opt.t, ag.critic_opt.t) == (2, 2, 2) and ag.critic_opt.lr == 1e-3
    for name in ("encoder", "actor", "critic", "critic_target"):
        for k, v in getattr(ag, name).state_dict().items():
            assert torch.equal(v, st[name][k]), (name, k)
    for net, on in (("enc", "encoder_opt"), ("actor", "actor_opt"), ("critic", "critic_opt")):
        for i, off in enumerate(eng.layout[net]):
            m = st[on]["state"][i]["exp_avg"].reshape(-1)
            assert torch.equal(eng.adam_m[off:off + m.numel()], m)
            assert torch.equal(eng.adam_v[off:off + m.numel()], st[on]["state"][i]["exp_avg_sq"].reshape(-1))
            assert bool(m.abs().sum() > 0)
    exp = ag.export_reference_state()
    for name in ("encoder", "actor", "critic", "critic_target"):
        assert all(torch.equal(exp[name][k], st[name][k]) for k in st[name])
    for on in ("encoder_opt", "actor_opt", "critic_opt"):
        assert exp[on]["state"].keys() == st[on]["state"].keys()
        for i, e in exp[on]["state"].items():
            assert float(e["step"]) == float(st[on]["state"][i]["step"]) == 2.0
            assert torch.equal(e["exp_avg"], st[on]["state"][i]["exp_avg"])
            assert torch.equal(e["exp_avg_sq"], st[on]["state"][i]["exp_avg_sq"])
    # the export is what a genuine torch.optim.Adam takes (the reference's optimisers are exactly that, drqv2.py:148-150)
    import io
    buf = io.BytesIO()
    torch.save(exp, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)                      # nothing but tensors and python scalars inside
    twin = drqv2.Critic(32 * 35 * 35, (d["A"],), d["F"], d["H"])
    twin.load_state_dict(back["critic"])
    opt = torch.optim.Adam(twin.parameters(), lr=5e-4)
    opt.load_state_dict(back["critic_opt"])
    assert opt.param_groups[0]["lr"] == 1e-3
    s0 = opt.state[next(iter(twin.parameters()))]
    assert float(s0["step"]) == 2.0 and torch.equal(s0["exp_avg"], st["critic_opt"]["state"][0]["exp_avg"])


def test_c_abi_exports_every_declared_symbol():
    """include/drqv2_hip.h <-> libdrqv2_hip.so <-> the ctypes prototype table."""
    from drqv2_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "drqv2_hip.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(drq_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert set(_lib.PROTOTYPES) == declared
    assert lib.drq_abi_version() == 7
    # ... and the other direction: the product library exports NOTHING named drq* beyond the header (internal helpers
    # have hidden visibility)
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    exported_drq = {n for n in exported if "drq" in n.lower()}
    assert exported_drq == declared, sorted(exported_drq ^ declared)
    # no environment knobs in the product library: update() cannot be steered onto an ablation by a stray variable
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    assert not any(ln.split()[-1].split("@")[0] in ("getenv", "secure_getenv") for ln in und.stdout.splitlines() if ln.strip())
    # layout entry points are host-only and callable without a GPU
    lay = _lib.param_layout(9, 6, 50, 1024)
    assert lay["seg"]["enc"][0] == 0 and lay["total"] == lay["seg"]["target"][1]
    n_enc = 32 * 9 * 9 + 32 + 3 * (32 * 32 * 9 + 32)
    assert lay["seg"]["enc"][1] >= n_enc
    assert lib.drq_step_ws_bytes(256, 9, 6, 50, 1024) > 0
    assert lib.drq_step_ws_bytes(0, 9, 6, 50, 1024) == 0
    # argument errors are reported, not executed (no GPU needed: the check precedes any launch)
    assert lib.drq_gemm_f32(None, 1, 1, None, 1, 1, None, 1, 4, 4, 4, 1, 0, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 0,
                            None, 0, None) == -1
    assert lib.drq_conv3x3_fwd(None, None, None, None, 1, 9, 84, 2, 1, 1, 1, 1, 0, None) == -1


def test_every_prototype_is_its_declaration():
    """restype and every argtype of every entry of _lib.PROTOTYPES against include/drqv2_hip.h (tests/abi.py holds the
    mapping); with the set equality above nothing is left uncompared"""
    from drqv2_amd import _lib
    from tests import abi
    assert len(abi.declarations()) > 90
    for name in abi.declarations():
        abi.assert_prototype(name)
    # launch() tells a stream entry from the rest by this list
    assert _lib.NO_STREAM == set(abi.declarations()) - abi.stream_entries()


def test_descriptor_enums_and_layout_length_are_the_headers():
    from drqv2_amd import _lib
    from tests import abi
    fields = abi.struct_fields("DrqStep")
    assert [f for f, _ in _lib.DrqStep._fields_] == [f for f, _ in fields]
    for (name, ctype), (_, allowed) in zip(_lib.DrqStep._fields_, fields):
        assert ctype in allowed, f"DrqStep.{name} is {ctype}, the header says {allowed}"
    enums = abi.enumerators()
    ws = {k[len("DRQ_WS_"):]: v for k, v in enums.items() if k.startswith("DRQ_WS_")}
    assert ws.pop("NBUF_PUBLIC") == len(_lib.WS_IDS)
    assert ws == {name: i for i, name in enumerate(_lib.WS_IDS)}
    phases = {k[len("DRQ_"):]: v for k, v in enums.items() if k.startswith("DRQ_PHASE_")}
    assert phases and phases == {k: v for k, v in vars(_lib).items() if k.startswith("PHASE_")}
    assert _lib.PARAM_LAYOUT_LEN == abi.define("DRQ_PARAM_LAYOUT_LEN")


@pytest.fixture
def no_stream(monkeypatch):
    """launch() without a GPU: the stream lookup gives the null stream"""
    from drqv2_amd import _lib
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    return _lib


def test_launch_checks_the_status_and_names_the_entry(no_stream):
    _lib = no_stream
    # the library refuses before any launch (tests/test_cpu_vec_eval.py relies on the same)
    with pytest.raises(_lib.DrqError, match="drq_vec_stack_push.*DRQ_EARG"):
        _lib.launch("drq_vec_stack_push", None, None, None, None, 1, 1)


@pytest.mark.parametrize("name", ["drq_no_such_entry", "drq_param_layout"])
def test_launch_takes_stream_entries_only(no_stream, monkeypatch, name):
    _lib = no_stream
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("launch() reached the library"))
    with pytest.raises(_lib.DrqError, match=name):
        _lib.launch(name, 9, 6, 50, 1024, None, 0)


@pytest.mark.parametrize("kw,entry", [({}, "drq_conv1_aug_fwd"), ({"bf16": True}, "drq_conv1_aug_fwd_bf16"),
                                      ({"bf16": True, "y_nhwc": True}, "drq_conv1_aug_fwd_bf16_nhwc")])
def test_conv1_aug_fwd_names_the_entry_it_called(no_stream, monkeypatch, kw, entry):
    from drqv2_amd import ops
    _lib, called = no_stream, []

    class Stub:
        def __getattr__(self, name):
            assert name.startswith("drq_conv1_aug_fwd"), name
            return lambda *args: called.append(name) or -1

    monkeypatch.setattr(_lib, "load", Stub)
    monkeypatch.setattr(ops, "_need", lambda t, *a, **k: t)     # the wrapper's own rule: GPU tensors only
    obs = torch.zeros((1, 9, 84, 84), dtype=torch.uint8)
    w, b, shift = torch.zeros(32, 9, 3, 3), torch.zeros(32), torch.zeros(1, 2)
    with pytest.raises(_lib.DrqError, match=entry + ":"):
        ops.conv1_aug_fwd(obs, shift, obs, shift, w, b, **kw)
    assert called == [entry]


def test_config_surface_matches_reference_yaml():
    from drqv2_amd import tasks
    with open(os.path.join(G, "cfg_surface.json")) as f:
        surf = json.load(f)
    assert sorted(tasks.TASKS) == sorted(surf["tasks"])
    for name, ref in surf["tasks"].items():
        cfg = tasks.resolve(name)
        for k in ("lr", "feature_dim", "stddev_schedule", "batch_size", "nstep", "num_train_frames", "frame_stack",
                  "action_repeat", "discount", "replay_buffer_size", "task_name"):
            want = float(ref[k]) if k == "lr" else ref[k]      # PyYAML reads the YAML 1e-4 as a string
            assert cfg[k] == want, (name, k, cfg[k], ref[k])
        for k, v in ref["agent"].items():
            if isinstance(v, str) and v.startswith("${"):
                continue
            if v == "???":
                continue
            assert cfg["agent"][k] == v, (name, k)
        kw = tasks.agent_kwargs(name, obs_shape=(9, 84, 84), action_shape=(6,), device="cpu")
        assert kw["lr"] == float(ref["lr"]) and kw["feature_dim"] == ref["feature_dim"]
        assert kw["stddev_schedule"] == ref["stddev_schedule"]


def test_schedule_and_helpers_match_reference():
    import utils
    with open(os.path.join(G, "schedule.json")) as f:
        ref = json.load(f)
    for s, vals in ref.items():
        for st, v in zip((0, 1, 999, 50000, 100000, 3000000), vals):
            assert float(utils.schedule(s, st)) == pytest.approx(v, rel=1e-15, abs=0)
    with pytest.raises(NotImplementedError):
        utils.schedule("cosine(1,2)", 3)
    u, e = utils.Until(100, 2), utils.Every(10, 2)
    assert u(49) and not u(50) and e(0) and e(5) and not e(6)
    assert utils.Until(None)(10 ** 9) and not utils.Every(None)(0)
    m = torch.nn.Linear(3, 3)
    with utils.eval_mode(m):
        assert not m.training
    assert m.training
