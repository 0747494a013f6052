"""The poisoned-memory harness (tests/poison.py) must be able to fail.  CPU tensors, plain Python functions standing in
for kernels: a correct writer passes; each of five defective ones is reported, with the right tensor named."""
import pytest
import torch

from tests import poison

ROWS, COLS = 7, 13


@pytest.fixture(autouse=True)
def clean_registry():
    poison.reset()
    yield
    poison.reset()


def raw(t, start, n):
    """n elements of t's storage from flat offset `start` relative to t (what a kernel's pointer arithmetic reaches)"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + start)


def k_correct(x, y):
    y.copy_(2 * x)


def k_skips_last_row(x, y):
    y[:-1].copy_(2 * x[:-1])


def k_skips_one_interior_element(x, y):
    keep = y[3, 5].clone()
    y.copy_(2 * x)
    y[3, 5] = keep


def k_stores_one_past_the_end(x, y):
    y.copy_(2 * x)
    raw(y, y.numel(), 1).fill_(1.0)


def k_stores_one_before_the_start(x, y):
    y.copy_(2 * x)
    raw(y, -1, 1).fill_(1.0)


def k_sums_one_past_the_input(x, y):
    y.copy_(2 * x)
    y[0, 0] = raw(x, 0, x.numel() + 1).sum()          # the last term is the first guard element behind x


def run(kernel):
    x = poison.put(torch.arange(ROWS * COLS, dtype=torch.float32).view(ROWS, COLS) + 1, name="x")
    y = poison.alloc((ROWS, COLS), torch.float32, "cpu", name="y")
    kernel(x, y)
    return x, y


def test_correct_writer_passes():
    x, y = run(k_correct)
    assert poison.report() == []
    poison.check()
    assert torch.equal(y, 2 * x)


def test_skipped_last_row_is_reported():
    run(k_skips_last_row)
    (f,) = poison.report()
    assert f.name.startswith("y ") and "never written" in f.what and f.count == COLS
    assert f.first[0] == ((ROWS - 1) * COLS, (ROWS - 1, 0)) and f.last == (ROWS * COLS - 1, (ROWS - 1, COLS - 1))
    with pytest.raises(AssertionError, match=r"y \[out float32\[7, 13\]\]: 13 element\(s\) never written"):
        poison.check()


def test_skipped_interior_element_is_reported():
    run(k_skips_one_interior_element)
    (f,) = poison.report()
    assert f.name.startswith("y ") and "never written" in f.what and f.count == 1
    assert f.first == [(3 * COLS + 5, (3, 5))]


def test_store_past_the_end_is_reported():
    run(k_stores_one_past_the_end)
    (f,) = poison.report()
    assert f.name.startswith("y ") and "AFTER" in f.what and f.count == 1 and f.first == [ROWS * COLS]
    with pytest.raises(AssertionError, match="guard band AFTER"):
        poison.check()


def test_store_before_the_start_is_reported():
    run(k_stores_one_before_the_start)
    (f,) = poison.report()
    assert f.name.startswith("y ") and "BEFORE" in f.what and f.count == 1 and f.first == [-1]


def test_read_past_the_end_of_an_input_is_reported():
    """The load itself leaves no trace; the value does: the sum is NaN, and with the sentinel's payload."""
    x, y = run(k_sums_one_past_the_input)
    fs = poison.report()
    assert len(fs) == 1 and fs[0].name.startswith("y ") and fs[0].count == 1 and fs[0].first == [(0, (0, 0))]
    assert "guard-band memory" in fs[0].what or "NaN" in fs[0].what
    assert bool(torch.isnan(y[0, 0]))
    # the same writer on an input that ends where the sum ends is clean: the report above is about the over-read
    poison.reset()
    x = poison.put(torch.ones(ROWS * COLS + 1), name="x")
    y = poison.alloc((ROWS, COLS), torch.float32, "cpu", name="y")
    k_sums_one_past_the_input(x[:ROWS * COLS].view(ROWS, COLS), y)
    poison.check()


def test_a_computed_nan_is_told_apart_from_an_unwritten_element():
    y = poison.alloc((4,), torch.float32, "cpu", name="y")
    y.copy_(torch.tensor([1.0, float("nan"), float("inf") - float("inf"), 2.0]))
    (f,) = poison.report()
    assert "never written" not in f.what and f.what.startswith("NaN") and f.count == 2 and f.first == [1, 2]


def test_inputs_workspaces_and_partly_written_outputs_only_have_their_guards_checked():
    poison.put(torch.zeros(5), name="in")
    poison.alloc((9,), torch.float32, "cpu", name="ws", kind="ws")
    z = poison.alloc((3, 3), torch.float32, "cpu", name="z", kind="zero")
    assert not bool(z.any())                                     # zeroed, as the wrappers hand such buffers out
    p = poison.partial(poison.alloc((6,), torch.float32, "cpu", name="p"))
    p[:2] = 1.0
    poison.check()
    raw(z, 9, 1).fill_(0.0)
    (f,) = poison.report()
    assert f.name.startswith("z ") and "AFTER" in f.what


def test_uint8_outputs_skip_the_written_check_but_keep_their_guards():
    u = poison.alloc((5,), torch.uint8, "cpu", name="u")
    poison.check()                                               # every byte is a legal value: nothing to tell
    raw(u, 5, 1).fill_(0)                                        # the byte right behind an odd-sized payload is guard
    (f,) = poison.report()
    assert "AFTER" in f.what and f.first == [5]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int64, torch.float64,
                                   torch.int32])
@pytest.mark.parametrize("shape", [(1,), (3, 5), (2, 3, 7, 7), (257,)])
def test_alloc_returns_contiguous_aligned_views_full_of_the_sentinel(dtype, shape):
    base = torch.empty(1 << 20, dtype=torch.uint8).data_ptr() % 64       # what the allocator itself guarantees here
    v = poison.alloc(shape, dtype, "cpu")
    assert v.dtype == dtype and tuple(v.shape) == shape and v.is_contiguous()
    rec = poison._records[-1]
    assert (v.data_ptr() - rec.raw.data_ptr()) == poison.GUARD and poison.GUARD % 256 == 0
    assert v.data_ptr() % 64 == base
    isz = v.element_size()
    assert rec.raw.numel() >= 2 * poison.GUARD + v.numel() * isz
    ints = v.view(-1).view(poison._INT[isz])
    assert bool((ints == poison.sentinel_of(dtype)).all())
    if v.is_floating_point():
        assert bool(torch.isnan(v).all())                                 # a used over-read cannot stay finite
    if isz == 4:
        assert poison.sentinel_of(dtype) == poison.SENTINEL == 0x7FC0DEAD
    v2 = poison.put(torch.zeros(shape, dtype=dtype))
    assert v2.dtype == dtype and tuple(v2.shape) == shape and v2.is_contiguous() and not bool(v2.any())
    with pytest.raises(ValueError):
        poison.alloc(shape, dtype, "cpu", guard=100)


def test_fixture_routes_and_restores_the_ops_allocation_function():
    """poisoned_ops is poisoning() around a test: inside, ops allocates poisoned memory; afterwards, pass or fail, the
    module's own function is back and nothing stays recorded."""
    from drqv2_amd import ops
    orig = ops._alloc
    with poison.poisoning():
        assert ops._alloc is not orig
        t = ops._alloc((4, 4), torch.float32, "cpu")
        assert bool(torch.isnan(t).all()) and len(poison._records) == 1 and "ops." in poison._records[0].name
        z = ops._alloc((4,), torch.float32, "cpu", "zero")
        assert not bool(z.any())
        t.zero_()
    assert ops._alloc is orig and poison._records == []
    with pytest.raises(AssertionError, match="never written"):
        with poison.poisoning():
            ops._alloc((4,), torch.float32, "cpu")                  # never written
    assert ops._alloc is orig and poison._records == []
    # a call the library refuses: the wrapper raises and drops its outputs, which must then be untouched, not written
    from drqv2_amd._lib import DrqError
    chk = ops.check
    with poison.poisoning():
        t = ops._alloc((4,), torch.float32, "cpu")
        with pytest.raises(DrqError):
            ops.check(-1, "refused")
        assert "refused" in poison._records[0].name
        u = ops._alloc((4,), torch.float32, "cpu")
        u.zero_()
        ops.check(0, "ok")
    with pytest.raises(AssertionError, match="written although the entry refused"):
        with poison.poisoning():
            t = ops._alloc((4,), torch.float32, "cpu")
            t[1] = 0.0
            with pytest.raises(DrqError):
                ops.check(-1, "refused")
    assert ops.check is chk
    with pytest.raises(ZeroDivisionError):
        with poison.poisoning():
            1 / 0
    assert ops._alloc is orig and poison._records == []
    # the default is plain torch: uninitialised or zeroed memory of the requested type
    e = orig((2, 3), torch.bfloat16, "cpu")
    assert e.dtype == torch.bfloat16 and tuple(e.shape) == (2, 3)
    assert not bool(orig((5,), torch.float32, "cpu", "zero").any())
