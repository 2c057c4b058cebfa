"""The slice splits and 64-pixel workgroups of the expand conv alone (hawq_conv_expand_reduce with reduce.wgt == NULL, fused_wp.hip):
every variant the library reports - one slice per workgroup and two-wave workgroups included - against the CPU oracle and, byte for
byte, against variant 1; with and without the stored residual, int8 and hawq4 block inputs, tie-free and exact-tie tables; the
subsampled forms (out_sub, res_sub) on an odd map; the overflow flag from a workgroup with blockIdx.y > 0.  Every buffer sits between
the guard bands of tests/guard.py, which are checked after every launch."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.guard import guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_fused import _case
from tests.test_gpu_kernels import dev, lib, orc, stream, unpack_q  # noqa: F401
from tests.test_gpu_out_sub import S, _launch_sub, _nibble_table, _solo_case, _sub
from tests.test_gpu_res_sub import _launch_res_sub, _small_input

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]

# (N, H, W, C, C3).  (3, 9, 7, ...): M = 189, the last 64- and 128-pixel tiles are partly empty; (2, 7, 7, ...): M = 98
SHAPES = [(2, 14, 14, 64, 256), (3, 9, 7, 128, 512), (1, 14, 14, 256, 1024), (2, 7, 7, 512, 2048)]
POISON = 0xAB


def _shapes(lib, a, nvar):
    """(pixels per workgroup, slice split) of variants 1..nvar."""
    out = []
    for v in range(1, nvar + 1):
        px, ys = C.c_int32(), C.c_int32()
        assert lib.load().hawq_conv_expand_reduce_variant_shape(C.byref(a), v, C.byref(px), C.byref(ys)) == 0, v
        out.append((px.value, ys.value))
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tie", [False, True])
def test_every_variant_equals_the_oracle_and_variant_1(lib, orc, guard_arena, shape, tie):  # noqa: F811
    n, h, w, c, c3 = shape
    a, keep, o, _ = _case(lib, orc, n, h, w, c, c3, zlib.crc32(repr(shape).encode()) + 21, force_tie=tie)
    a.reduce = lib.ExpandReduceArgs().reduce   # zeroed: the expand conv alone
    ex = a.expand
    nvar = lib.load().hawq_conv_expand_reduce_variants(C.byref(a))
    shapes = _shapes(lib, a, nvar)
    assert shapes[0] == (128, 1) and all((c3 // 64) % ys == 0 for _, ys in shapes) and len(set(shapes)) == nvar
    res_ref = np.ascontiguousarray(o.transpose(0, 2, 3, 1)).astype(np.uint16)
    mq4, eq4, q4_ref = _nibble_table(orc, o)
    mq8, eq8 = ex.mq, ex.eq
    for bits, q_ref in ((8, keep['q_ref']), (4, q4_ref)):
        ex.out_bits, ex.q_lo, ex.q_hi = (8, 0, 127) if bits == 8 else (4, 0, 15)
        ex.mq, ex.eq = (mq8, eq8) if bits == 8 else (mq4, eq4)
        assert lib.load().hawq_conv_expand_reduce_variants(C.byref(a)) == nvar
        qbuf = out_buf(o.size * bits // 8, torch.uint8, POISON)
        ex.out_q = qbuf.data_ptr()
        for with_res in (True, False):
            ex.res_out = keep['res_out'].data_ptr() if with_res else None
            first = None
            for tile in range(1, nvar + 1):
                a.tile = tile
                keep['res_out'].view(torch.uint8).fill_(0x5A), qbuf.fill_(POISON), keep['flags'].zero_()
                lib.call("hawq_conv_expand_reduce", C.byref(a), stream())
                guard_arena.check()
                got = (keep['res_out'].cpu().numpy().reshape(n, h, w, c3), qbuf.cpu().numpy())
                what = (bits, with_res, tile, shapes[tile - 1])
                assert keep['flags'].item() == 0, what   # the oracle's residual stays below 65536 (asserted in _case)
                assert np.array_equal(got[0], res_ref if with_res else np.full_like(res_ref, 0x5A5A)), what
                assert np.array_equal(unpack_q(qbuf, (n, h, w, c3), bits), q_ref), what
                if first is None:
                    first = got
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), what
    ex.mq, ex.eq = mq8, eq8


@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_subsampled_forms_on_an_odd_map(lib, orc, guard_arena, c):  # noqa: F811
    """out_sub = 2 and the res_sub form of the same launch: a 9 x 7 source map, a 5 x 4 dense grid, two images (M' = 40: an image
    boundary inside the first wave tile, a partly empty 64-pixel workgroup)."""
    shape = (2, 9, 7)
    n, h, w = shape
    c3 = 4 * c
    assert (_sub(h), _sub(w)) == (5, 4)
    a, keep, o = _solo_case(lib, orc, c, shape, False)
    keep['x2s'] = _small_input(keep, shape, c)
    ex = a.expand
    nvar = lib.load().hawq_conv_expand_reduce_variants(C.byref(a))
    assert nvar == len(_shapes(lib, a, nvar))
    mq4, eq4, q4_ref = _nibble_table(orc, o)
    mq8, eq8 = ex.mq, ex.eq
    for bits, q_ref in ((8, keep['q_ref']), (4, q4_ref)):
        row_bytes = c3 * bits // 8
        ex.out_bits, ex.q_lo, ex.q_hi = (8, 0, 127) if bits == 8 else (4, 0, 15)
        ex.mq, ex.eq = (mq8, eq8) if bits == 8 else (mq4, eq4)
        want = q_ref[:, :, ::S, ::S]
        first = None
        for tile in range(1, nvar + 1):
            a.tile = tile
            for form, got in (("out_sub", _launch_sub(lib, "hawq_conv_expand_reduce", a, ex, shape, row_bytes, (bits, tile))),
                              ("res_sub", _launch_res_sub(lib, "hawq_conv_expand_reduce", a, ex, keep, shape, row_bytes, (bits, tile)))):
                guard_arena.check()
                q = unpack_q(torch.from_numpy(np.ascontiguousarray(got).reshape(-1)), (n, _sub(h), _sub(w), c3), bits)
                assert np.array_equal(q, want), (bits, tile, form)
                first = got if first is None else first
                assert np.array_equal(got, first), (bits, tile, form)
                assert keep['flags'].item() == 0
    ex.mq, ex.eq = mq8, eq8


def test_overflow_flag_from_a_workgroup_behind_the_first(lib, orc, guard_arena):  # noqa: F811
    """After test_expand_reduce_overflow_flag: one stored residual above 65535, in the LAST 64-channel slice - with any split it belongs
    to a workgroup with blockIdx.y > 0 -, raises the flag in every variant; the same values without a stored residual raise nothing
    (the flag reports a saturated store, and the block input is computed from the un-clamped sum)."""
    n, h, w, c, c3 = 1, 7, 7, 256, 1024
    a, keep, o, _ = _case(lib, orc, n, h, w, c, c3, 6)
    a.reduce = lib.ExpandReduceArgs().reduce
    qbuf = out_buf(o.size, torch.uint8, 0)
    a.expand.out_q = qbuf.data_ptr()
    res = np.zeros((n, h, w, c3), np.uint16)
    pixel, ch = (0, 3, 5), c3 - 7
    res[pixel + (ch,)] = 65535
    keep['res'] = dev(res)
    a.expand.res_in = keep['res'].data_ptr()
    a.expand.m_id_scalar, a.expand.e_id_scalar = 1 << 30, 33 | (5 << 8)   # (v << 5) * 2^30 / 2^33 = 4 v: 262 140 > 65 535 at that one element
    nvar = lib.load().hawq_conv_expand_reduce_variants(C.byref(a))
    shapes = _shapes(lib, a, nvar)
    assert max(ys for _, ys in shapes) >= 4   # (the last slice is then never the first workgroup's)
    for tile in range(1, nvar + 1):
        a.tile = tile
        for with_res in (True, False):
            a.expand.res_out = keep['res_out'].data_ptr() if with_res else None
            keep['flags'].zero_(), keep['res_out'].zero_()
            lib.call("hawq_conv_expand_reduce", C.byref(a), stream())
            guard_arena.check()
            assert keep['flags'].item() == int(with_res), (tile, shapes[tile - 1], with_res)
            if with_res:   # the carrier saturates at that element and nowhere else
                got = keep['res_out'].cpu().numpy().reshape(n, h, w, c3)
                assert got[pixel + (ch,)] == 65535 and int((got == 65535).sum()) == 1, tile
