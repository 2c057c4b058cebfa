"""Host side of the split-K grouped InceptionV3 conv launch (hawq_amd/csrc/incep_splitk.hip): hawq_incep_conv_group_splitk_ok and
hawq_incep_conv_group_splitk_workspace on fabricated pointers (nothing is dereferenced).  No GPU needed."""
import ctypes as C

import pytest

from hawq_amd import _lib
from tests.test_incep_group_host import RQ2, Fab, concat, group, member

R = _lib.INCEP_RAW


def _ok(members, slices, tile=3):
    return _lib.load().hawq_incep_conv_group_splitk_ok(C.byref(group(members)), tile, (C.c_int32 * 8)(*slices))


def _concat_level(fab, n=2):
    """the four members of the kernel test's concat_level: slices 0 .. 64 and 160 .. 192 of one int16 buffer, int8, RAW - with Cin 256
    (4 steps) where the grouped launch's case has Cin 64: one step cannot be cut into the 2 and 4 slices the case asks for"""
    cat = fab.buf()
    return [member(fab, 8, 8, 256, 64, n=n, epilogue=RQ2, out_bits=16, out=cat, ldo=192, c_off=0), member(fab, 8, 8, 256, 48, n=n),
            member(fab, 8, 8, 256, 96, n=n, epilogue=R, out_bits=32), member(fab, 8, 8, 256, 32, n=n, epilogue=RQ2, out_bits=16, out=cat, ldo=192, c_off=160)]


@pytest.mark.parametrize("slices,want", [(1, 0), (2, 1), (3, 1), (4, 0), (5, 1), (6, 0), (0, 0), (33, 0), (-1, 0)])
def test_no_empty_slice_on_five_steps(slices, want):
    """Cin 320, 1x1: 5 steps.  S = 3 is q = 2 (2 + 2 + 1); S = 4 is q = 2 as well and leaves slice 3 empty; S = 1 alone is no split"""
    assert _ok([member(Fab(), 8, 8, 320, 80)], [slices]) == want


def test_slice_count_range_and_tiles():
    fab = Fab()
    long_k = [member(fab, 8, 8, 448, 384, 3, 3, 1, 1)]   # 63 steps
    assert _ok(long_k, [32]) == 1 and _ok(long_k, [33]) == 0 and _ok(long_k, [0]) == 0
    assert [_ok(long_k, [16], t) for t in range(6)] == [0, 0, 0, 1, 0, 0]
    assert _ok(_concat_level(fab), [1, 2, 4, 1]) == 1 and _ok(_concat_level(fab), [1, 1, 1, 1]) == 0
    # the grouped launch's refusals: nine members, overlapping members
    g, two = group([member(fab, 5, 5, 128, 16) for _ in range(8)]), (C.c_int32 * 8)(*[2] * 8)
    assert _lib.load().hawq_incep_conv_group_splitk_ok(C.byref(g), 3, two) == 1
    g.n = 9
    assert _lib.load().hawq_incep_conv_group_splitk_ok(C.byref(g), 3, two) == 0
    assert _ok(concat(fab, 192, [(0, 64), (64, 96)], 8, 8, 128), [2, 2]) == 1
    assert _ok(concat(fab, 192, [(0, 64), (48, 96)], 8, 8, 128), [2, 2]) == 0


@pytest.mark.parametrize("n", [1, 3])
def test_workspace_of_the_concat_level(n):
    """P = 64 n: one pixel block at n = 1, two at n = 3; channel blocks 1, 1, 2, 1; only members 1 and 2 are split"""
    L, slab, cnt = _lib.load(), C.c_int64(-1), C.c_int64(-1)
    g, s = group(_concat_level(Fab(), n)), (C.c_int32 * 8)(1, 2, 4, 1)
    assert L.hawq_incep_conv_group_splitk_workspace(C.byref(g), 3, s, C.byref(slab), C.byref(cnt)) == 0
    npb = -(-64 * n // 128)
    assert slab.value == (npb * 1 * 2 + npb * 2 * 4) * 128 * 64 * 4 and cnt.value == 4 * (npb * 1 + npb * 2)
    s[2] = 5   # four steps: the fifth slice would be empty
    assert L.hawq_incep_conv_group_splitk_workspace(C.byref(g), 3, s, C.byref(slab), C.byref(cnt)) != 0
    assert b"member 2" in L.hawq_last_error() and b"empty slice" in L.hawq_last_error()
    assert L.hawq_incep_conv_group_splitk(C.byref(g), 3, s, 16, None, None) != 0   # refused on the host, before any launch
