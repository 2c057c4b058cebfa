"""Host side of the mixed-form grouped launch: hawq_incep_conv_group_nib_ok (arithmetic on made-up addresses, nothing is dereferenced)
and the engine option's precondition.  No GPU."""
import ctypes as C

import pytest

from tests.test_gpu_incep_group_nib_kernels import A, blocks_for, group
from tests.test_gpu_incep_nib_kernels import REQUANT, _block, _lib

# made-up addresses, 16-byte aligned and far apart: (in, wgt, bias, out, m, ek) of members A and B (one output row) and C
AB, OC = 0x4000000, 0x5000000
FAKE = [(0x1000000 * (i + 1), 0x100000, 0x200000, out, 0x300000, 0x300000) for i, out in enumerate((AB, AB, OC))]


def _ok(blocks, mask, tile):
    return bool(_lib().load().hawq_incep_conv_group_nib_ok(C.byref(group(blocks)), mask, tile))


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("mask", [0b000, 0b111, 0b101, 0b010])
def test_ok_takes_the_three_member_group(mask, tile):
    assert _lib().load().hawq_incep_conv_group_nib_num_tiles() == 2
    assert _ok(blocks_for(FAKE, mask), mask, tile) and _ok(blocks_for(FAKE, mask, raw=True), mask, tile)


def test_ok_refuses_other_tiles_stray_mask_bits_and_nibble_stores_of_int8_members():
    b = blocks_for(FAKE, 0b111)   # C stores nibbles
    assert _ok(b, 0b111, 2)
    assert not _ok(b, 0b111, 3) and not _ok(b, 0b111, 0)
    assert not _ok(b, 0b1111, 2) and not _ok(b[:2], 0b100, 2)
    assert not _ok(b, 0b011, 2)   # out_bits 4, and C is int8 in this mask


def test_extents_are_those_of_the_real_byte_widths():
    """X's input ends, as hawq4 (Cin / 2 bytes a pixel), exactly where Y's output begins; as int8 it would run on into it"""
    n_in = 2 * 9 * 9 * 48
    x = _block(A, (0x1000000, 0x100000, 0x200000, 0x2000000, 0x300000, 0x300000), REQUANT, 8, q=(-128, 127))
    y = _block(A, (0x6000000, 0x100000, 0x200000, 0x1000000 + n_in // 2, 0x300000, 0x300000), REQUANT, 8, q=(-128, 127))
    assert _ok([x, y], 0b01, 2) and _ok([x, y], 0b11, 2)
    assert not _ok([x, y], 0b00, 2) and not _ok([x, y], 0b10, 2)
    # an out_bits 4 output is half a byte an element: Y ends where Z's input begins only if it stores nibbles
    n_out = 2 * 9 * 9 * 80
    z = _block(A, (0x7000000 + n_out // 2, 0x100000, 0x200000, 0x8000000, 0x300000, 0x300000), REQUANT, 8, q=(-128, 127))
    y4 = _block(A, (0x6000000, 0x100000, 0x200000, 0x7000000, 0x300000, 0x300000), REQUANT, 4, q=(0, 15))
    y8 = _block(A, (0x6000000, 0x100000, 0x200000, 0x7000000, 0x300000, 0x300000), REQUANT, 8, q=(-128, 127))
    assert _ok([y4, z], 0b01, 2) and not _ok([y8, z], 0b01, 2)


def _why(blocks, mask, tile):
    """the reason hawq_incep_conv_group_nib gives for refusing the group (it is refused on the host, before any launch)"""
    L = _lib().load()
    assert L.hawq_incep_conv_group_nib(C.byref(group(blocks)), mask, tile, None) != 0
    return L.hawq_last_error().decode()


@pytest.mark.parametrize("tile", [1, 2])
def test_neighbouring_nibble_slices_of_one_row_are_independent_until_they_overlap(tile):
    from tests.test_gpu_incep_group_nib_kernels import LDO_ROW, ROW, row_blocks
    ptrs = [(0x1000000, 0x100000 * (i + 1), 0x200000, AB, 0x300000, 0x300000) for i in range(3)]   # one input, one output row buffer
    assert _ok(row_blocks(ptrs), 0b111, tile)
    overlap = "two members write overlapping outputs"
    middle_moved = (ROW[0], (16, 32), ROW[2])      # onto the first member's slice
    first_widened = ((16, 32), ROW[1], ROW[2])     # into the middle member's
    for row in (middle_moved, first_widened):
        assert not _ok(row_blocks(ptrs, row), 0b111, tile) and overlap in _why(row_blocks(ptrs, row), 0b111, tile)
    # One member stores 8 bits through the same base pointer: it is no slice of the nibble rows any more (another element width), and its
    # bytes, 96 a pixel from byte 64 on, cover its neighbours' nibbles.  The extents are compared in bytes worked out in half bytes.
    for i in range(3):
        bits = tuple(8 if j == i else 4 for j in range(3))
        assert not _ok(row_blocks(ptrs, bits=bits), 0b111, tile) and overlap in _why(row_blocks(ptrs, bits=bits), 0b111, tile)
    # ... and the nibble rows end where half bytes say: 162 pixels of 48 bytes.  An 8-bit member from there on is independent of them;
    # one row earlier it is not.
    end = AB + 162 * LDO_ROW // 2
    for out, ok in ((end, True), (end - LDO_ROW // 2, False)):
        moved = [ptrs[0], ptrs[1], ptrs[2][:3] + (out,) + ptrs[2][4:]]
        assert bool(_ok(row_blocks(moved, (ROW[0], ROW[1], (0, 16)), (4, 4, 8)), 0b111, tile)) == ok


def test_nibble_groups_needs_nibble():
    from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable
    with pytest.raises(PlanNotApplicable, match="nibble_groups"):
        InceptionEngine(None, nibble_groups=True)
