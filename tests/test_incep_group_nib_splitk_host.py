"""Host side of the mixed-form split-K grouped InceptionV3 conv launch (hawq_amd/csrc/incep_group_nib_splitk.hip):
hawq_incep_conv_group_nib_splitk_ok and hawq_incep_conv_group_nib_splitk_workspace on fabricated pointers (nothing is dereferenced).
No GPU needed."""
import ctypes as C

import pytest

from hawq_amd import _lib
from tests.test_incep_group_host import RQ, RQ2, Fab, group, member

R = _lib.INCEP_RAW


def _ok(members, mask, slices, tile=2):
    return _lib.load().hawq_incep_conv_group_nib_splitk_ok(C.byref(group(members)), mask, tile, (C.c_int32 * 8)(*slices))


def mixed_level(fab, n=1):
    """the kernel test's mixed_level (mask 0b1010): int8 RQ2 and hawq4 RQ2 into slices 0 .. 64 and 160 .. 192 of one int16 buffer,
    a hawq4 member that stores nibbles, an int8 RAW member; Cin 256: 4 int8 steps, 2 hawq4 steps"""
    cat = fab.buf()
    nib4 = member(fab, 8, 8, 256, 48, n=n, epilogue=RQ, out_bits=4)
    nib4.q_hi = 15
    return [member(fab, 8, 8, 256, 64, n=n, epilogue=RQ2, out_bits=16, out=cat, ldo=192, c_off=0), nib4,
            member(fab, 8, 8, 256, 96, n=n, epilogue=R, out_bits=32), member(fab, 8, 8, 256, 32, n=n, epilogue=RQ2, out_bits=16, out=cat, ldo=192, c_off=160)]


@pytest.mark.parametrize("mask,slices,want", [(1, 1, 0), (1, 2, 1), (1, 3, 1), (1, 4, 0), (0, 4, 0), (0, 5, 1), (0, 6, 0), (1, 0, 0), (1, 33, 0)])
def test_steps_follow_the_members_form(mask, slices, want):
    """Cin 320, 1x1: 20 units are 3 hawq4 steps (S = 2: 2 + 1, S = 3: one each, S = 4: q = 1 and an empty slice) and 5 int8 steps"""
    assert _ok([member(Fab(), 8, 8, 320, 80)], mask, [slices]) == want


def test_tiles_masks_and_forms():
    fab = Fab()
    assert [_ok([member(fab, 8, 8, 320, 80)], 1, [2], t) for t in range(4)] == [0, 0, 1, 0]
    assert _ok(mixed_level(fab), 0b1010, [1, 2, 4, 1]) == 1 and _ok(mixed_level(fab), 0b1010, [1, 1, 1, 1]) == 0
    assert _ok(mixed_level(fab), 0b1010, [1, 3, 4, 1]) == 0   # two hawq4 steps have no third slice
    assert _ok(mixed_level(fab), 0b11010, [1, 2, 4, 1]) == 0  # a mask bit beyond n
    assert _ok(mixed_level(fab), 0b1000, [1, 2, 4, 1]) == 0   # member 1 stores nibbles but is int8 in this mask


@pytest.mark.parametrize("n", [1, 3])
def test_workspace_of_the_mixed_level(n):
    """P = 64 n: one pixel block at n = 1, two at n = 3; channel blocks 1, 1, 2, 1; only members 1 and 2 are split"""
    L, slab, cnt = _lib.load(), C.c_int64(-1), C.c_int64(-1)
    g, s = group(mixed_level(Fab(), n)), (C.c_int32 * 8)(1, 2, 4, 1)
    assert L.hawq_incep_conv_group_nib_splitk_workspace(C.byref(g), 0b1010, 2, s, C.byref(slab), C.byref(cnt)) == 0, L.hawq_last_error()
    npb = -(-64 * n // 128)
    assert slab.value == (npb * 1 * 2 + npb * 2 * 4) * 128 * 64 * 4 and cnt.value == 4 * (npb * 1 + npb * 2)
    s[1] = 3
    assert L.hawq_incep_conv_group_nib_splitk_workspace(C.byref(g), 0b1010, 2, s, C.byref(slab), C.byref(cnt)) != 0
    assert b"member 1" in L.hawq_last_error() and b"empty slice" in L.hawq_last_error()
    assert L.hawq_incep_conv_group_nib_splitk(C.byref(g), 0b1010, 2, s, None, None, None) != 0   # refused on the host, before any launch
