"""Guard-banded test buffers: every tensor a kernel test hands to a kernel sits between two poisoned guards.

``GuardArena.put`` / ``GuardArena.empty`` return views into a backing slab of their own,

    [ lead guard | view | round-up to 256 B | tail guard ]

whose guards are ``guard`` bytes of ``poison`` each and belong to that buffer alone, so a changed byte names one
buffer and one side.  Views start on a 256-byte boundary (the kernels ask for 16), and the bytes between the end of
a view and the next 256-byte boundary count as tail guard.  ``check()`` synchronises and asserts that every guard
byte still holds the poison.

What this sees
  * a store outside a buffer, up to ``guard`` bytes away from it.  The default of 1 MiB is a condition, not a
    measurement: it covers a full 256-pixel tile of the widest row these tests use (2048 channels x 2 B of uint16
    residual carrier).  A stray store further away than that is out of reach.
  * a result that depends on bytes outside an input: those bytes are the poison, not the zeros of fresh device
    memory that happen to equal the correct padding, so the oracle comparison of the test itself fails.

What it does not see
  * a stray store of the poison value itself.  tests/test_gpu_guard_edges.py runs every case with two poisons.
  * an over-read whose value never reaches a result.  No buffer is placed at the end of a mapping, nothing is
    arranged so that an over-read faults: such a read is not detectable here and is out of scope.

Module-level ``dev`` / ``out_buf`` allocate from the arena the ``guard_arena`` fixture made current, and plainly on
the GPU when none is.  This is a plain module: a test file imports the fixture to use it.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

ALIGN = 256
_current = None


class GuardError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "slab", "start", "nbytes", "end")

    def __init__(self, name, slab, start, nbytes, end):
        self.name, self.slab, self.start, self.nbytes, self.end = name, slab, start, nbytes, end


class GuardArena:
    def __init__(self, device, poison=0xA5, guard=1 << 20):
        assert 0 <= poison <= 255 and guard > 0
        self.device, self.poison, self.guard = torch.device(device), int(poison), int(guard)
        self.bufs = []
        self.peak_bytes = 0

    # ------------------------------------------------------------------ allocation
    def _carve(self, nbytes, name):
        g = self.guard
        span = -(-nbytes // ALIGN) * ALIGN
        slab = torch.full((g + ALIGN + span + g,), self.poison, dtype=torch.uint8, device=self.device)
        if self.device.type == "cuda":   # the fill is done before a launch on any other stream (the engines own theirs) can use the view
            torch.cuda.current_stream(self.device).synchronize()
        start = -(slab.data_ptr() + g) % ALIGN + g   # first 256-byte boundary with a whole guard in front of it
        b = _Buf(name or f"buf{len(self.bufs)}", slab, start, nbytes, slab.numel())
        self.bufs.append(b)
        self.peak_bytes = max(self.peak_bytes, sum(x.slab.numel() for x in self.bufs))
        return b, slab[start:start + nbytes]

    def empty(self, n, dtype, name=None, fill=None):
        """A view of ``n`` elements (an int or a shape) of ``dtype``; holds the poison unless ``fill`` is given."""
        shape = (int(n),) if isinstance(n, (int, np.integer)) else tuple(int(v) for v in n)
        count = int(np.prod(shape, dtype=np.int64))
        _, raw = self._carve(count * torch.empty(0, dtype=dtype).element_size(), name)
        v = raw.view(dtype).reshape(shape)
        if fill is not None:
            if fill == 0:
                v.zero_()
            else:
                v.fill_(fill)
        return v

    def put(self, a, name=None):
        """Upload a numpy array or a tensor; the view has its shape and dtype."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        t = t.contiguous()
        _, raw = self._carve(t.numel() * t.element_size(), name)
        raw.copy_(t.reshape(-1).view(torch.uint8))
        return raw.view(t.dtype).reshape(t.shape)

    # ------------------------------------------------------------------ checking
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _changed(self, bufs):
        total = None
        for b in bufs:
            c = (b.slab[:b.start] != self.poison).sum() + (b.slab[b.start + b.nbytes:b.end] != self.poison).sum()
            total = c if total is None else total + c
        return 0 if total is None else int(total.item())

    def _report(self, bufs):
        lines = []
        for b in bufs:
            s = b.slab.cpu().numpy()
            for side, lo, hi, rel in (("lead", 0, b.start, b.start), ("tail", b.start + b.nbytes, b.end, b.start)):
                bad = np.flatnonzero(s[lo:hi] != self.poison)
                if bad.size:
                    off = lo + int(bad[0]) - rel
                    lines.append(f"buffer '{b.name}' ({b.nbytes} B): {side} guard changed, {bad.size} byte(s), first at "
                                 f"offset {off} relative to the buffer (value 0x{int(s[lo + bad[0]]):02x}, poison "
                                 f"0x{self.poison:02x})")
        return lines

    def check(self, bufs=None):
        """Synchronise, then assert that every guard byte (of ``bufs``, default all) still equals the poison."""
        bufs = self.bufs if bufs is None else bufs
        self._sync()
        if self._changed(bufs):
            raise GuardError("guard bytes changed:\n  " + "\n  ".join(self._report(bufs)))

    def release(self, *views):
        """Check the guards of these views now and give their memory back (for tests that walk through many large
        buffers).  The views must not be used afterwards."""
        ptrs = {v.data_ptr() for v in views if v.numel()}
        gone = [b for b in self.bufs if b.nbytes and b.slab.data_ptr() + b.start in ptrs]
        self.check(gone)
        self.bufs = [b for b in self.bufs if b not in gone]


# ---------------------------------------------------------------------- the current arena
def current():
    return _current


def set_current(arena):
    global _current
    prev, _current = _current, arena
    return prev


@pytest.fixture
def guard_arena():
    """Every dev() / out_buf() of the test comes from one arena; its guards are checked when the test ends."""
    arena = GuardArena("cuda")
    prev = set_current(arena)
    try:
        yield arena
    finally:
        set_current(prev)
    arena.check()


def dev(a, name=None):
    if _current is not None:
        return _current.put(a, name)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def out_buf(n, dtype, fill, name=None):
    """``n`` elements (an int or a shape) of ``dtype``: ``fill`` None leaves them unset, else sets them."""
    if _current is not None:
        return _current.empty(n, dtype, name, fill)
    shape = (int(n),) if isinstance(n, (int, np.integer)) else tuple(n)
    if fill is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def release(*views):
    """Drop large buffers early (see GuardArena.release); without an arena the caller's ``del`` does that."""
    if _current is not None:
        _current.release(*views)
