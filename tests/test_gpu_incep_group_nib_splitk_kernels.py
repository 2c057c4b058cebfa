"""The mixed-form split-K grouped InceptionV3 conv launch (hawq_amd/csrc/incep_group_nib_splitk.hip, hawq_incep_conv_group_nib_splitk)
against a plain int64 convolution with the exact dyadic requant, and byte for byte against hawq_incep_conv_group_nib on tile 2, in
guard-banded, sentinel-filled buffers, on a slab pre-filled with garbage and on the workspace the first launch left.  The cases are
the smallest shapes at which cutting K on nibble rows can go wrong (steps: 64-byte rows, eight 16-channel units of a hawq4 member)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (the fixture)
from tests.test_gpu_incep_group_nib_kernels import BOUNDS, _tables, _want, group
from tests.test_gpu_incep_nib_kernels import RAW, REQUANT, REQUANT2, _block, _case, _lib

pytestmark = pytest.mark.gpu
TWO = dict(m2=5 << 27, ek2=31, q2=(-16384, 16383), relu=1)   # 5/16, ties of its own


def _m(g, epilogue=REQUANT, bits=8, out=None, ldo=None, c_off=0):
    """a member: geometry (KH, KW, pad_h, pad_w, stride, H, W, Cin, Cout), epilogue, store width, shared buffer name, its pitch, slice"""
    return dict(g=g, epilogue=epilogue, bits=bits, out=out, ldo=ldo or g[8], c_off=c_off)


LONG = _m((3, 3, 1, 1, 1, 8, 8, 448, 384), REQUANT2, 16)    # 252 units, 32 hawq4 steps
STRADDLE = _m((3, 3, 1, 1, 1, 9, 9, 48, 16))                # 27 units, 4 steps: slices start mid-tap, the last step has 3 units
# name -> (members, mask, slice counts per run)
CASES = {
    "uneven": ([_m((1, 1, 0, 0, 1, 8, 8, 640, 80))], 0b1, [(2,), (3,), (5,)]),            # 5 steps: 3 + 2, 2 + 2 + 1, one each
    "straddle": ([STRADDLE], 0b1, [(2,), (4,)]),
    "rect_17": ([_m((1, 7, 0, 3, 1, 17, 17, 160, 160)), _m((7, 1, 3, 0, 1, 17, 17, 160, 192))], 0b11, [(3, 5)]),   # 9 steps, P = 289 N
    "mixed_level": ([_m((1, 1, 0, 0, 1, 8, 8, 256, 64), REQUANT2, 16, "cat", 192, 0), _m((1, 1, 0, 0, 1, 8, 8, 256, 48), REQUANT, 4),
                     _m((1, 1, 0, 0, 1, 8, 8, 256, 96), RAW, 32), _m((1, 1, 0, 0, 1, 8, 8, 256, 32), REQUANT2, 16, "cat", 192, 160)],
                    0b1010, [(1, 2, 4, 1)]),
    "long": ([LONG], 0b1, [(7,), (16,)]),                    # q = 5: a slice crosses into the register-held chunk, the last is 2 steps; q = 2
    "long_unsplit": ([LONG, STRADDLE], 0b11, [(1, 2)]),      # 32 steps through the chunked loop, beside a small split member
}
PARAMS = [pytest.param(name, s, id=f"{name}-{'_'.join(map(str, s))}") for name, (_, _, runs) in CASES.items() for s in runs]
DT = {4: torch.uint8, 8: torch.int8, 16: torch.int16, 32: torch.int32}


def _images(a, N):
    """`_case` makes two images: the first alone, or the two and the first again"""
    return a[:1] if N == 1 else np.concatenate([a, a[:1]])


def _buffers(members, N):
    bufs = {}
    for i, mb in enumerate(members):
        g, key = mb["g"], mb["out"] or f"out{i}"
        P = N * ((g[5] + 2 * g[2] - g[0]) // g[4] + 1) * ((g[6] + 2 * g[3] - g[1]) // g[4] + 1)
        if key not in bufs:
            bufs[key] = out_buf(P * mb["ldo"] // (2 if mb["bits"] == 4 else 1), DT[mb["bits"]], 0x77 if mb["bits"] == 4 else 77, key)
    return bufs


def _operands(members, mask, N):
    """per member (in, wgt, bias, m, ek) on the device in the form its mask bit names, and (reference, m, ek) on the host"""
    from hawq_amd.packing import pack_conv_weight, pack_hawq4
    ptrs, host = [], []
    for i, mb in enumerate(members):
        x, w, b, ref = _case(mb["g"])
        x, ref, nib = _images(x, N), _images(ref, N), (mask >> i) & 1
        m, e = _tables(ref, mb["bits"])
        t = [dev(pack_hawq4(x) if nib else x.astype(np.int8), f"x{i}"), dev(pack_conv_weight(w.transpose(0, 3, 1, 2), 4 if nib else 8), f"w{i}"),
             dev(b.astype(np.int32), f"b{i}"), dev(m, f"m{i}"), dev(e, f"ek{i}")]
        ptrs.append([v.data_ptr() for v in t])
        host.append((ref, m, e))
    return ptrs, host


def _blocks(members, ptrs, bufs, N):
    out = []
    for i, (mb, p) in enumerate(zip(members, ptrs)):
        o = bufs[mb["out"] or f"out{i}"].data_ptr()
        kw = TWO if mb["epilogue"] == REQUANT2 else dict(relu=int(mb["bits"] == 4))
        out.append(_block(mb["g"], (p[0], p[1], p[2], o, p[3], p[4]), mb["epilogue"], mb["bits"], mb["ldo"], mb["c_off"],
                          q=BOUNDS.get(mb["bits"], (0, 0)), N=N, **kw))
    return out


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name,slices", PARAMS)
def test_split_launch_equals_int64_conv_and_the_mixed_group_launch(guard_arena, name, slices, N):   # noqa: F811
    from hawq_amd.packing import unpack_hawq4
    L, (members, mask, _), st = _lib().load(), CASES[name], torch.cuda.current_stream().cuda_stream
    ptrs, host = _operands(members, mask, N)
    first, second, plain = _buffers(members, N), _buffers(members, N), _buffers(members, N)
    g, s = group(_blocks(members, ptrs, first, N)), (C.c_int32 * 8)(*slices)
    want = [_want(a, ref, m, e) for a, (ref, m, e) in zip(g.conv, host)]
    assert all(a.epilogue == RAW or len(np.unique(w)) >= 4 for a, w in zip(g.conv, want))   # no degenerate requant: several levels
    assert L.hawq_incep_conv_group_nib_splitk_ok(C.byref(g), mask, 2, s) == 1
    sb, cb = C.c_int64(), C.c_int64()
    assert L.hawq_incep_conv_group_nib_splitk_workspace(C.byref(g), mask, 2, s, C.byref(sb), C.byref(cb)) == 0, L.hawq_last_error()
    slab, counters = out_buf(sb.value, torch.uint8, 0x5b, "slab"), out_buf(cb.value // 4, torch.int32, 0, "counters")
    assert L.hawq_incep_conv_group_nib_splitk(C.byref(g), mask, 2, s, slab.data_ptr(), counters.data_ptr(), st) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    assert not counters.any()
    g2 = group(_blocks(members, ptrs, second, N))   # the workspace as the first launch left it
    assert L.hawq_incep_conv_group_nib_splitk(C.byref(g2), mask, 2, s, slab.data_ptr(), counters.data_ptr(), st) == 0, L.hawq_last_error()
    assert L.hawq_incep_conv_group_nib(C.byref(group(_blocks(members, ptrs, plain, N))), mask, 2, st) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    assert not counters.any()
    for key in plain:
        assert torch.equal(first[key], plain[key]), f"buffer {key} differs from the mixed-form grouped launch's"
        assert torch.equal(second[key], plain[key]), f"buffer {key} of the second launch differs"
    for i, (mb, a, w) in enumerate(zip(members, g.conv, want)):
        got = first[mb["out"] or f"out{i}"].cpu().numpy().reshape(w.shape[0] * w.shape[1] * w.shape[2], -1)
        got = unpack_hawq4(got) if mb["bits"] == 4 else got.astype(np.int64)
        assert np.array_equal(got[:, a.c_off:a.c_off + a.Cout], w.reshape(-1, a.Cout)), f"member {i} differs from the int64 convolution"


@pytest.mark.parametrize("name,mask,slices,tile,bits,why", [
    ("rect_17", 0b11, (3, 4), 2, None, b"empty slice"), ("mixed_level", 0b1010, (1, 1, 1, 1), 2, None, b"more than one slice"),
    ("uneven", 0b1, (2,), 1, None, b"tile 2"), ("uneven", 0b11, (2,), 2, None, b"beyond n"), ("uneven", 0b0, (2,), 2, 4, b"int8 member")])
def test_a_refused_call_is_an_error_and_writes_nothing(guard_arena, name, mask, slices, tile, bits, why):   # noqa: F811
    L, members = _lib().load(), [dict(mb, bits=bits or mb["bits"]) for mb in CASES[name][0]]
    bufs = _buffers(members, 1)
    p = dev(np.zeros(1 << 16, np.int32), "operands").data_ptr()   # stands for every operand: a refused call reads none
    g, s = group(_blocks(members, [[p] * 5] * len(members), bufs, 1)), (C.c_int32 * 8)(*slices)
    slab, counters = out_buf(1 << 20, torch.uint8, 0x5b, "slab"), out_buf(64, torch.int32, 0, "counters")
    assert L.hawq_incep_conv_group_nib_splitk_ok(C.byref(g), mask, tile, s) == 0
    rc = L.hawq_incep_conv_group_nib_splitk(C.byref(g), mask, tile, s, slab.data_ptr(), counters.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and why in L.hawq_last_error(), L.hawq_last_error()
    torch.cuda.synchronize()
    assert all((t == (0x77 if t.dtype == torch.uint8 else 77)).all() for t in bufs.values()) and (slab == 0x5b).all() and not counters.any()
