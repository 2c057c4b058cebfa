"""The guard-band detector of tests/guard.py, proved on a CPU arena (no GPU needed): what it must catch, whom it
must blame, and its one documented blind spot."""
import numpy as np
import pytest
import torch

from tests import guard as G

GUARD = 4096


def arena(**kw):
    kw.setdefault("guard", GUARD)
    return G.GuardArena("cpu", **kw)


def slab_of(ar, view):
    """(backing slab, offset of the view in it) - the way a stray store reaches the bytes around a view."""
    for b in ar.bufs:
        if b.slab.data_ptr() + b.start == view.data_ptr():
            return b.slab, b.start
    raise KeyError


def fails(ar):
    with pytest.raises(G.GuardError) as ei:
        ar.check()
    return str(ei.value)


def test_untouched_arena_passes_and_views_are_aligned():
    ar = arena()
    a = ar.put(np.arange(7, dtype=np.int32), "a")
    b = ar.empty(5, torch.uint16, "b", fill=0)
    c = ar.empty((3, 11), torch.float32, "c", fill=float("nan"))
    d = ar.empty(13, torch.uint8, "d")
    e = ar.put(torch.arange(6, dtype=torch.int16).reshape(2, 3), "e")
    assert a.tolist() == list(range(7)) and a.dtype == torch.int32
    assert b.dtype == torch.uint16 and int(b.to(torch.int32).sum()) == 0
    assert c.shape == (3, 11) and bool(torch.isnan(c).all())
    assert (d == 0xA5).all()   # unset memory is poison, not zero
    assert e.shape == (2, 3) and e.tolist() == [[0, 1, 2], [3, 4, 5]]
    for v in (a, b, c, d, e):
        assert v.data_ptr() % 256 == 0
    ar.check()


def test_default_guard_is_one_mebibyte_each_side():
    ar = G.GuardArena("cpu")
    v = ar.put(np.zeros(3, np.uint8), "v")
    slab, off = slab_of(ar, v)
    assert ar.guard == 1 << 20 and off >= 1 << 20 and slab.numel() - (off + 256) >= 1 << 20
    ar.check()
    slab[-1] = 0
    assert "'v'" in fails(ar)


def test_byte_directly_before_a_view_is_a_lead_hit():
    ar = arena()
    ar.put(np.ones(40, np.uint8), "first")
    v = ar.put(np.ones(100, np.uint8), "victim")
    slab, off = slab_of(ar, v)
    slab[off - 1] = 0
    msg = fails(ar)
    assert "'victim'" in msg and "lead" in msg and "offset -1 " in msg and "1 byte(s)" in msg
    assert "'first'" not in msg and "tail" not in msg


def test_byte_directly_behind_a_view_is_a_tail_hit():
    ar = arena()
    v = ar.put(np.ones(256, np.uint8), "victim")   # ends on the 256-byte boundary: the very next byte is tail guard
    slab, off = slab_of(ar, v)
    slab[off + 256] = 7
    msg = fails(ar)
    assert "'victim'" in msg and "tail" in msg and "offset 256 " in msg and "lead" not in msg


def test_far_ends_of_both_guards_are_watched():
    for where in ("lead", "tail"):
        ar = arena()
        v = ar.put(np.ones(100, np.uint8), "victim")
        slab, off = slab_of(ar, v)
        idx = off - GUARD if where == "lead" else off + 256 + GUARD - 1
        slab[idx] = 0
        msg = fails(ar)
        assert "'victim'" in msg and where in msg


def test_alignment_round_up_behind_a_view_is_guard():
    ar = arena()
    v = ar.put(np.ones(100, np.uint8), "victim")
    slab, off = slab_of(ar, v)
    slab[off + 100] = 0   # first byte past the view, well before the next 256-byte boundary
    slab[off + 255] = 0
    msg = fails(ar)
    assert "'victim'" in msg and "tail" in msg and "offset 100 " in msg and "2 byte(s)" in msg


def test_writes_inside_views_pass():
    ar = arena()
    a = ar.empty(100, torch.int32, "a", fill=-7)
    b = ar.put(np.zeros((4, 5), np.float32), "b")
    a[:] = 3
    a[0], a[-1] = 1, 2
    b.fill_(1.5)
    ar.check()
    assert a[-1] == 2 and float(b.sum()) == 30.0


def test_neighbours_are_attributed_correctly():
    ar = arena()
    a = ar.put(np.ones(64, np.uint8), "left")
    b = ar.put(np.ones(64, np.uint8), "right")
    sa, oa = slab_of(ar, a)
    sa[oa + 64 + 3] = 0   # behind "left"
    msg = fails(ar)
    assert "'left'" in msg and "tail" in msg and "'right'" not in msg
    ar = arena()
    a = ar.put(np.ones(64, np.uint8), "left")
    b = ar.put(np.ones(64, np.uint8), "right")
    sb, ob = slab_of(ar, b)
    sb[ob - 5:ob] = 0     # in front of "right"
    msg = fails(ar)
    assert "'right'" in msg and "lead" in msg and "offset -5 " in msg and "5 byte(s)" in msg and "'left'" not in msg
    sa, oa = slab_of(ar, a)
    sa[oa + 64] = 1       # now both: two lines, one per buffer
    msg = fails(ar)
    assert "'left'" in msg and "'right'" in msg


def test_a_store_of_the_poison_value_is_the_blind_spot():
    """Documented in tests/guard.py: a stray store of the poison itself changes nothing, so check() passes.  The
    directed GPU cases (tests/test_gpu_guard_edges.py) therefore run with two poisons, 0xA5 and 0x5A."""
    ar = arena(poison=0xA5)
    v = ar.put(np.ones(100, np.uint8), "v")
    slab, off = slab_of(ar, v)
    slab[off + 100] = 0xA5
    slab[off - 1] = 0xA5
    ar.check()
    ar2 = arena(poison=0x5A)   # the same store under the second poison is caught
    v = ar2.put(np.ones(100, np.uint8), "v")
    slab, off = slab_of(ar2, v)
    slab[off + 100] = 0xA5
    assert "tail" in fails(ar2)


def test_release_checks_and_forgets_a_buffer():
    ar = arena()
    a = ar.put(np.ones(64, np.uint8), "a")
    b = ar.put(np.ones(64, np.uint8), "b")
    sb, ob = slab_of(ar, b)
    ar.release(a)
    assert [x.name for x in ar.bufs] == ["b"]
    sb[ob - 1] = 0
    with pytest.raises(G.GuardError, match="'b'"):
        ar.release(b)


def test_module_helpers_use_the_current_arena():
    ar = arena()
    prev = G.set_current(ar)
    try:
        x = G.dev(np.arange(5, dtype=np.int8), "x")
        y = G.out_buf(9, torch.int32, -7)
        z = G.out_buf((2, 3), torch.uint8, None, "z")
    finally:
        G.set_current(prev)
    assert G.current() is prev
    assert x.device.type == "cpu" and x.tolist() == [0, 1, 2, 3, 4] and (y == -7).all() and z.shape == (2, 3)
    assert [b.name for b in ar.bufs] == ["x", "buf1", "z"]
    ar.check()
