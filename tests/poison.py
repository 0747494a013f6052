"""Poisoned, guarded memory for the op tests (a helper module: not collected, not a conftest).

A kernel test that allocates its result with torch.empty can pass without the kernel writing anything: the caching
allocator hands back the block a previous, correct call of the same shape has just freed.  And a store or a load a few
elements outside a tensor lands in the allocator's rounding slack or in a finite neighbour, where no comparison looks.
This module closes both holes:

  alloc(shape, dtype, device)   one flat allocation [guard | payload | guard], ALL of it filled with a sentinel; returns
                                the contiguous payload view and records the allocation
  put(t, device)                the same for an input: payload = a copy of t, guards = sentinel
  check()                       every guard band still holds the sentinel (no out-of-bounds store) and no element of a
                                recorded output still does (every element was written); raises with the tensor's name,
                                the count and the first / last indices
  poisoned_ops                  autouse fixture: drqv2_amd.ops allocates through alloc() while a test runs, then check()

The sentinel of a 4-byte element is SENTINEL = 0x7FC0DEAD: a quiet NaN whose payload no arithmetic produces from
ordinary operands (2-byte: 0x7FDE, a NaN in bf16 and fp16; 8-byte: 0x7FF8DEAD7FC0DEAD; 1-byte: 0xA5).  Comparisons
are made on the integer view, never on float values, so a NaN a kernel computed is told apart from an element it never
wrote.  An out-of-range LOAD cannot be seen directly, but what it reads is this NaN: if the value is used -- even
"times zero" -- the result is NaN.  The hardware propagates the payload of a NaN operand, so such an element usually
shows up in check() as "still the sentinel"; any other NaN in a float output is reported as well.

uint8 outputs: every byte value is a legal result, so the "was written" check is skipped for them (their guards are
checked like all others).
"""
import contextlib
import math
import sys
from collections import namedtuple

import pytest
import torch

SENTINEL = 0x7FC0DEAD
_SENT = {1: 0xA5, 2: 0x7FDE, 4: SENTINEL, 8: 0x7FF8DEAD7FC0DEAD}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
GUARD = 64 * 1024          # bytes on each side; any multiple of 256 keeps the payload's alignment

Finding = namedtuple("Finding", "name what count numel first last")
_Rec = namedtuple("_Rec", "name kind raw ints g_el numel view")
_records = []


def sentinel_of(dtype):
    """the integer whose bit pattern fills poisoned memory of this element type"""
    return _SENT[torch.empty((), dtype=dtype).element_size()]


def _caller(depth):
    f = sys._getframe(depth)
    while f.f_code.co_name.startswith("<") and f.f_back is not None:      # comprehensions have frames of their own
        f = f.f_back
    return f"{f.f_code.co_name}:{f.f_lineno}"


def alloc(shape, dtype=torch.float32, device="cpu", guard=GUARD, name=None, kind="out"):
    """kind: "out" = an output the kernel must write in full; "ws" = scratch (guards only); "zero" = partly written by
    contract (payload zeroed as the wrappers do, guards only); "in" = an input (guards only, see put); "refused" = an
    output of a call that returned an error: nothing may have been launched, every element must still be poison."""
    if guard <= 0 or guard % 256:
        raise ValueError("guard must be a positive multiple of 256 bytes")
    if kind not in ("out", "ws", "zero", "in", "refused"):
        raise ValueError(kind)
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    isz = torch.empty((), dtype=dtype).element_size()
    numel = math.prod(shape)
    nbytes = numel * isz
    total = 2 * guard + (nbytes + 255) // 256 * 256
    raw = torch.empty(total, dtype=torch.uint8, device=device)
    ints = raw.view(_INT[isz])
    ints.fill_(_SENT[isz])
    view = raw[guard:guard + nbytes].view(dtype).view(shape)
    if kind == "zero":
        view.zero_()
    name = name or _caller(2)
    _records.append(_Rec(f"{name} [{kind} {str(dtype).replace('torch.', '')}{list(shape)}]", kind, raw, ints, guard // isz,
                         numel, view))
    return view


def put(t, device=None, guard=GUARD, name=None):
    """a copy of t between two guard bands (an input: only the bands are checked)"""
    v = alloc(t.shape, t.dtype, t.device if device is None else device, guard, name or _caller(2), "in")
    v.copy_(t)
    return v


def _find(t):
    for i, r in enumerate(_records):
        if r.view.data_ptr() == t.data_ptr() and r.view.device == t.device:
            return i
    raise KeyError("not a tensor of alloc() / put()")


def partial(t):
    """mark a recorded output as partly written by contract: only its guards are checked from now on"""
    i = _find(t)
    _records[i] = _records[i]._replace(kind="zero", name=_records[i].name.replace("[out ", "[zero "))
    return t


def forget(t):
    _records.pop(_find(t))


def reset():
    del _records[:]
    _ops_mark[0] = 0


def _where(mask, shape):
    idx = mask.reshape(-1).nonzero().reshape(-1)
    n = int(idx.numel())
    first = [int(i) for i in idx[:4].tolist()]
    last = int(idx[-1])
    if shape is not None and len(shape) > 1:
        def unr(i):
            idx = []
            for d in reversed(shape):
                i, r = divmod(i, d)
                idx.append(r)
            return tuple(reversed(idx))
        return n, [(i, unr(i)) for i in first], (last, unr(last))
    return n, first, last


def report():
    """the list of Findings over everything recorded since the last reset()"""
    if any(r.raw.is_cuda for r in _records):
        torch.cuda.synchronize()
    out = []
    for r in _records:
        sent = _SENT[r.ints.element_size()]
        # guard elements are indexed relative to the tensor: -1 is the element right before it, numel the one right after
        for what, m, base in (("stored into the guard band BEFORE the tensor", r.ints[:r.g_el] != sent, -r.g_el),
                              ("stored into the guard band AFTER the tensor", r.ints[r.g_el + r.numel:] != sent, r.numel)):
            if bool(m.any()):
                n, first, last = _where(m, None)
                out.append(Finding(r.name, what, n, r.numel, [i + base for i in first], last + base))
        pay = r.ints[r.g_el:r.g_el + r.numel]
        if r.kind == "refused" and r.numel and bool((pay != sent).any()):
            n, first, last = _where(pay != sent, r.view.shape)
            out.append(Finding(r.name, "written although the entry refused the call", n, r.numel, first, last))
        if r.kind != "out" or r.numel == 0:
            continue
        if r.view.dtype != torch.uint8:
            stale = pay == sent
            if bool(stale.any()):
                n, first, last = _where(stale, r.view.shape)
                out.append(Finding(r.name, "never written, or computed from guard-band memory (still the sentinel)", n,
                                   r.numel, first, last))
            if r.view.is_floating_point():
                nan = torch.isnan(r.view).reshape(-1) & ~stale
                if bool(nan.any()):
                    n, first, last = _where(nan, r.view.shape)
                    out.append(Finding(r.name, "NaN (was a value from outside an operand used?)", n, r.numel, first, last))
    return out


def check():
    bad = report()
    if bad:
        raise AssertionError("poisoned-memory check failed:\n" + "\n".join(
            f"  {f.name}: {f.count} element(s) {f.what} (the tensor has {f.numel}); first {f.first}, last {f.last}"
            for f in bad))


def _ops_alloc(shape, dtype, device, kind="out"):
    return alloc(shape, dtype, device, name="ops." + _caller(2), kind=kind)


_ops_mark = [0]


def _ops_check(rc, what=""):
    """drqv2_amd.ops.check while poisoned: the outputs a wrapper allocated for a call the library then refused (it
    raises, nobody ever sees them) must not have been touched, instead of having been written in full"""
    from drqv2_amd import _lib
    if rc != 0:
        for i in range(min(_ops_mark[0], len(_records)), len(_records)):
            r = _records[i]
            if r.kind == "out" and r.name.startswith("ops."):
                _records[i] = r._replace(kind="refused", name=r.name.replace("[out ", "[refused "))
    _ops_mark[0] = len(_records)
    _lib.check(rc, what)


@contextlib.contextmanager
def poisoning():
    """drqv2_amd.ops takes every result and workspace from alloc() inside the block; at its end the device is
    synchronised and check() runs; the module's own allocation function is restored whatever happens."""
    from drqv2_amd import ops
    saved = ops._alloc, ops.check
    reset()
    ops._alloc, ops.check = _ops_alloc, _ops_check
    try:
        yield sys.modules[__name__]
        check()
    finally:
        ops._alloc, ops.check = saved
        reset()


@pytest.fixture(autouse=True)
def poisoned_ops():
    """poisoning() around every test of the module that imports this fixture"""
    with poisoning() as p:
        yield p
