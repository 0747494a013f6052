"""act_batch(): the public surface and the argument checks of its C entry, none of which needs a GPU (every error is
reported before any launch)."""
import inspect

from drqv2_amd import _lib

DRQ_EARG, DRQ_EWS = -1, -2


def test_agent_has_act_batch_with_the_documented_parameters():
    import drqv2
    fn = drqv2.DrQV2Agent.act_batch
    assert list(inspect.signature(fn).parameters) == ["self", "obs", "step", "eval_mode"]


def test_prototypes_list_the_new_entries():
    assert "drq_act_ws_bytes" in _lib.PROTOTYPES and "drq_act_batch" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.drq_abi_version() == 7           # the change is additive


def test_act_ws_bytes_domain():
    lib = _lib.load()
    assert lib.drq_act_ws_bytes(0, 9, 6, 50, 1024) == 0
    for dims in ((9, 6, 50, 1024), (9, 21, 100, 1024), (9, 3, 20, 64), (9, 6, 50, 256)):
        sizes = [lib.drq_act_ws_bytes(n, *dims) for n in (1, 16, 64)]
        assert all(s > 0 for s in sizes), (dims, sizes)
        assert sizes == sorted(sizes), (dims, sizes)
    assert lib.drq_act_ws_bytes(16, 12, 6, 50, 1024) == 0       # frame_stack 4: not built
    assert lib.drq_act_ws_bytes(16, 9, 6, 0, 1024) == 0
    assert lib.drq_act_ws_bytes(16, 9, 6, 257, 1024) == 0       # LayerNorm width: the engine's own limit
    assert lib.drq_act_ws_bytes(16, 9, 0, 50, 1024) == 0
    assert lib.drq_act_ws_bytes(-3, 9, 6, 50, 1024) == 0


def test_act_batch_argument_errors_come_before_any_launch():
    """No GPU is present here: a call that reached a launch would return a positive hipError_t (or crash on the
    fake pointers); every case below must be turned away by the argument checks."""
    lib = _lib.load()
    dims = (9, 6, 50, 1024)
    big = lib.drq_act_ws_bytes(16, *dims)
    fake = 0x1000                                               # never dereferenced

    def call(params=fake, obs=fake, n=4, noise=None, mu=None, action=fake, ws=fake, ws_bytes=big, d=dims):
        return lib.drq_act_batch(params, *d, obs, n, noise, 0.5, mu, action, ws, ws_bytes, None)

    assert call(params=None) == DRQ_EARG
    assert call(obs=None) == DRQ_EARG
    assert call(action=None) == DRQ_EARG
    assert call(ws=None) == DRQ_EARG
    assert call(n=0) == DRQ_EARG
    assert call(n=-1) == DRQ_EARG
    assert call(d=(12, 6, 50, 1024)) == DRQ_EARG
    assert call(d=(9, 6, 300, 1024)) == DRQ_EARG
    assert call(ws_bytes=0) == DRQ_EWS
    assert call(ws_bytes=lib.drq_act_ws_bytes(4, *dims) - 4) == DRQ_EWS
    assert call(n=17) == DRQ_EWS                                # n above the n_max the workspace was sized for
    assert call(n=100000) == DRQ_EARG                           # above what the kernels take at all
