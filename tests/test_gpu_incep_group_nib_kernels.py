"""The mixed-form grouped InceptionV3 conv launch (hawq_amd/csrc/incep_group_nib.hip, hawq_incep_conv_group_nib) against a plain int64
convolution and the exact dyadic requant: groups of three members, each as int8 or as hawq4, on both tiles, in guard-banded buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (the fixture)
from tests.test_gpu_incep_nib_kernels import RAW, REQUANT, REQUANT2, _block, _case, _lib
from tests.test_gpu_incep_tiled_kernels import _dyadic   # round_half_even(v m / 2^e) in exact integers

pytestmark = pytest.mark.gpu

# (KH, KW, pad_h, pad_w, stride, H, W, Cin, Cout), N = 2
A = (1, 1, 0, 0, 1, 9, 9, 48, 80)     # P = 162: two pixel blocks; Cout 80: a partial channel block; three units as hawq4, 3/4 LDS row as int8
B = (1, 7, 0, 3, 1, 6, 9, 48, 32)     # units of one slot in different taps, one in the padding; P = 108
C3 = (3, 3, 0, 0, 2, 9, 9, 80, 144)   # K = 720: both stages reused; P = 32; three channel blocks on tile 2, two on tile 1
MEMBERS = (A, B, C3)
LDO_AB, OFF_A, OFF_B = 160, 16, 112   # A and B share one row: channels 16 .. 95 and 112 .. 143 of 160
LDO_C, OFF_C = 144 + 48, 32
BOUNDS = {4: (0, 15), 8: (-128, 127), 16: (-32768, 32767)}


def group(blocks):
    g = _lib().IncepGroupArgs()
    g.n = len(blocks)
    for i, a in enumerate(blocks):
        g.conv[i] = a
    return g


def blocks_for(ptrs, mask, raw=False):
    """the three members' blocks on the pointers ``ptrs[i] = (in, wgt, bias, out, m, ek)``; C stores nibbles when it reads them"""
    if raw:
        return [_block(A, ptrs[0], RAW, 32, LDO_AB, OFF_A), _block(B, ptrs[1], RAW, 32, LDO_AB, OFF_B), _block(C3, ptrs[2], RAW, 32, LDO_C, OFF_C)]
    cb = 4 if mask & 4 else 8
    two = dict(m2=5 << 27, ek2=31, q2=(-16384, 16383), relu=1)   # 5/16, ties of its own
    return [_block(A, ptrs[0], REQUANT2, 16, LDO_AB, OFF_A, BOUNDS[16], **two), _block(B, ptrs[1], REQUANT2, 16, LDO_AB, OFF_B, BOUNDS[16], **two),
            _block(C3, ptrs[2], REQUANT, cb, LDO_C, OFF_C, BOUNDS[cb], relu=int(cb != 8))]


def _tables(ref, out_bits):
    """per-channel ratios that spread |ref| over the store's range, with exact ties on channel 0 (ratio 1/2: every odd value)"""
    cout = ref.shape[-1]
    m = np.random.default_rng(cout).integers(1 << 29, 1 << 30, cout).astype(np.int32)
    e = np.full(cout, 30 + max(int(np.abs(ref).max()).bit_length() - out_bits, 1), np.int32)
    m[0], e[0] = 1 << 30, 31
    return m, e


def _want(a, ref, m, e):
    if a.epilogue == RAW:
        return ref
    v = np.maximum(ref, 0) if a.relu else ref
    want = np.clip(np.stack([_dyadic(v[..., c], m[c], int(e[c])) for c in range(a.Cout)], -1), a.q_lo, a.q_hi)
    return np.clip(_dyadic(want, a.m2, a.ek2), a.q2_lo, a.q2_hi) if a.epilogue == REQUANT2 else want


@pytest.mark.parametrize("raw", [False, True], ids=["requant", "raw"])
@pytest.mark.parametrize("mask", [0b000, 0b111, 0b101, 0b010])
@pytest.mark.parametrize("tile", [1, 2])
def test_mixed_group_equals_int64_conv_and_requant(guard_arena, tile, mask, raw):   # noqa: F811
    from hawq_amd.packing import pack_conv_weight, pack_hawq4, unpack_hawq4
    L = _lib().load()
    cases = [_case(g) for g in MEMBERS]
    cbits = 32 if raw else 4 if mask & 4 else 8
    dt = {4: torch.uint8, 8: torch.int8, 16: torch.int16, 32: torch.int32}
    ab = out_buf(162 * LDO_AB, dt[32 if raw else 16], 77, "out_ab")
    oc = out_buf(32 * LDO_C // (2 if cbits == 4 else 1), dt[cbits], 0x77 if cbits == 4 else 77, "out_c")   # 0x77: two nibbles of 7
    ptrs, tabs = [], []
    for i, (g, (x, w, b, ref)) in enumerate(zip(MEMBERS, cases)):
        nib = (mask >> i) & 1
        xd = dev(pack_hawq4(x) if nib else x.astype(np.int8), f"x{i}")
        wd = dev(pack_conv_weight(w.transpose(0, 3, 1, 2), 4 if nib else 8), f"w{i}")
        m, e = _tables(ref, cbits if i == 2 else 16)
        tabs.append((m, e))
        ptrs.append((xd.data_ptr(), wd.data_ptr(), dev(b.astype(np.int32), f"b{i}").data_ptr(), (oc if i == 2 else ab).data_ptr(),
                     dev(m, f"m{i}").data_ptr(), dev(e, f"ek{i}").data_ptr()))
    blocks = blocks_for(ptrs, mask, raw)
    assert L.hawq_incep_conv_group_nib(C.byref(group(blocks)), mask, tile, torch.cuda.current_stream().cuda_stream) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    want = [_want(a, ref, m, e).reshape(-1, a.Cout) for a, (_, _, _, ref), (m, e) in zip(blocks, cases, tabs)]
    assert raw or all(len(np.unique(w)) >= 4 for w in want)   # no degenerate requant: several levels in every member
    got = ab.cpu().numpy().reshape(162, LDO_AB).astype(np.int64)
    exp = np.full_like(got, 77)
    exp[:162, OFF_A:OFF_A + 80], exp[:108, OFF_B:OFF_B + 32] = want[0], want[1]
    assert np.array_equal(got, exp)   # both slices, and the sentinel everywhere else: the gaps, and B's columns below its 108 rows
    got = oc.cpu().numpy().reshape(32, -1)
    got = unpack_hawq4(got) if cbits == 4 else got.astype(np.int64)
    exp = np.full_like(got, 7 if cbits == 4 else 77)
    exp[:, OFF_C:OFF_C + 144] = want[2]
    assert np.array_equal(got, exp)


# Three hawq4 members on A's map writing neighbouring nibble slices of one row, as the plan's concat buffers are written: channels
# 16 .. 31, 32 .. 63 and 64 .. 79 of 96, a 16-channel gap of sentinel on either side.  Member i convolves rows ROW_W[i] of A's weights.
LDO_ROW = 96
ROW = ((16, 16), (32, 32), (64, 16))               # (c_off, Cout)
ROW_W = (slice(0, 16), slice(16, 48), slice(48, 64))
# different forms and clamps, so that a store landing in a neighbour's bytes changes a value there
ROW_FORMS = (dict(epilogue=REQUANT, q=(0, 15), relu=1), dict(epilogue=REQUANT2, q=(0, 15), m2=5 << 27, ek2=31, q2=(1, 14), relu=1),
             dict(epilogue=REQUANT, q=(3, 12), relu=0))


def row_blocks(ptrs, row=ROW, bits=(4, 4, 4)):
    """the three members' blocks on ``ptrs[i] = (in, wgt, bias, out, m, ek)``; ``row`` and ``bits`` are what the host test varies"""
    return [_block(A[:8] + (cout,), ptrs[i], out_bits=bits[i], ldo=LDO_ROW, c_off=c_off, **ROW_FORMS[i]) for i, (c_off, cout) in enumerate(row)]


@pytest.mark.parametrize("tile", [1, 2])
def test_neighbouring_nibble_slices_of_one_row(guard_arena, tile):   # noqa: F811
    from hawq_amd.packing import pack_conv_weight, pack_hawq4, unpack_hawq4
    L = _lib().load()
    x, w, b, ref = _case(A)
    P = 162
    out = out_buf(P * LDO_ROW // 2, torch.uint8, 0x77, "row")   # 0x77: two nibbles of 7
    xd = dev(pack_hawq4(x), "x")
    ptrs, tabs = [], []
    for i, ((c_off, cout), rows) in enumerate(zip(ROW, ROW_W)):
        r = ref[..., rows]
        m = np.random.default_rng(100 + i).integers(1 << 29, 1 << 30, cout).astype(np.int32)
        e = np.full(cout, 30 + max(int(np.abs(r).max()).bit_length() - 6, 1), np.int32)   # the larger sums pass the upper clamp
        m[0], e[0] = 1 << 30, 31   # ratio 1/2: every odd value an exact tie
        tabs.append((m, e))
        ptrs.append((xd.data_ptr(), dev(pack_conv_weight(w[rows].transpose(0, 3, 1, 2), 4), f"w{i}").data_ptr(),
                     dev(b[rows].astype(np.int32), f"b{i}").data_ptr(), out.data_ptr(), dev(m, f"m{i}").data_ptr(), dev(e, f"ek{i}").data_ptr()))
    blocks = row_blocks(ptrs)
    assert L.hawq_incep_conv_group_nib(C.byref(group(blocks)), 0b111, tile, torch.cuda.current_stream().cuda_stream) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    exp = np.full((P, LDO_ROW), 7, np.int64)
    for a, rows, (m, e) in zip(blocks, ROW_W, tabs):
        want = _want(a, ref[..., rows], m, e).reshape(P, a.Cout)
        assert len(np.unique(want)) >= 4 and want.min() == (a.q2_lo if a.epilogue == REQUANT2 else a.q_lo)   # several levels, the lower edge
        exp[:, a.c_off:a.c_off + a.Cout] = want
    got = unpack_hawq4(out.cpu().numpy().reshape(P, LDO_ROW // 2)).astype(np.int64)
    assert np.array_equal(got, exp)   # the three slices, and the sentinel in both gaps


def test_a_refused_group_is_an_error_and_writes_nothing(guard_arena):   # noqa: F811
    L = _lib().load()
    ab, oc = out_buf(162 * LDO_AB, torch.int16, 77, "out_ab"), out_buf(32 * LDO_C, torch.int8, 77, "out_c")
    p = dev(np.zeros(1 << 16, np.int32), "operands").data_ptr()   # large enough to stand for every operand
    ptrs = [(p, p, p, ab.data_ptr(), p, p), (p, p, p, ab.data_ptr(), p, p), (p, p, p, oc.data_ptr(), p, p)]
    ok = blocks_for(ptrs, 0b011)
    reads = blocks_for([ptrs[0], ptrs[1], (ab.data_ptr(), p, p, oc.data_ptr(), p, p)], 0b011)   # C reads what A and B write
    nib8 = blocks_for(ptrs, 0b111)                                                             # C stores nibbles ...
    for blocks, mask, n in ((reads, 0b011, 3), (ok, 0b1011, 3), (ok[:2], 0b100, 2), (nib8, 0b011, 3)):   # ... but is int8 in this mask
        g = group(blocks[:n])
        assert not L.hawq_incep_conv_group_nib_ok(C.byref(g), mask, 2)
        assert L.hawq_incep_conv_group_nib(C.byref(g), mask, 2, torch.cuda.current_stream().cuda_stream) != 0 and L.hawq_last_error()
    assert L.hawq_incep_conv_group_nib_ok(C.byref(group(ok)), 0b011, 2)   # the refusals above are not the shapes'
    torch.cuda.synchronize()
    assert (ab == 77).all() and (oc == 77).all()
