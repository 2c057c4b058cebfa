"""hawq_conv_args.out_sub (include/hawq_mi355.h): a 1x1 expand launch that evaluates only the output pixels (n, s y', s x') the
next stage's stride-s 1x1 convs read, and stores them densely.  The wave-private solo kernel (fused_wp.hip) and hawq_conv2d's general
tiles take it; every byte must equal the out_sub = 0 launch gathered at [:, ::s, ::s], nothing may be written behind the M' dense
rows, and every other kernel family must refuse the field through its applicability query."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.guard import guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_fused import _case
from tests.test_gpu_kernels import dev, lib, nhwc, odyadic, orc, stream, unpack_q  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]

S = 2
# (n, h, w): odd map with M' = 32 (an image boundary inside the single wave tile); non-square with M' = 45 (ragged last wave tile);
# M' = 125, one short of a 128-pixel workgroup
SHAPES = [(2, 7, 7), (3, 6, 10), (5, 9, 9)]
CHANNELS = [64, 128, 256]
POISON, TAIL = 0xAB, 4096


def _sub(n):
    return (n - 1) // S + 1


def _solo_case(lib, orc, c, shape, tie):
    n, h, w = shape
    a, keep, o, _ = _case(lib, orc, n, h, w, c, 4 * c, zlib.crc32(repr((c, shape)).encode()) + 11, force_tie=tie)
    a.reduce = lib.ExpandReduceArgs().reduce   # the expand conv alone
    a.expand.res_out = None                    # out_sub launches write no residual (the next unit is a resize unit)
    return a, keep, o


def _nibble_table(orc, o):
    """A 4-bit next QuantAct that clamps ~30 % of the outputs (as tests/test_gpu_fused.py draws it)."""
    from hawq_amd.quant_utils import requant_table
    r4 = 15.0 / max(1.0, float(np.percentile(o, 70)))
    mq4, eq4 = requant_table(torch.tensor([r4 * 0.7], dtype=torch.float32), torch.ones(1), torch.tensor([0.7]))
    return int(mq4[0]), int(eq4[0]), odyadic(orc, o, mq4, eq4, (0, 15))


def _dense_rows(buf, shape, row_bytes):
    n, h, w = shape
    return buf.cpu().numpy()[:n * h * w * row_bytes].reshape(n, h, w, row_bytes)


def _launch_sub(lib, entry, args, conv, shape, row_bytes, what):
    """Launch `entry` with conv.out_sub = S into a poisoned buffer: (the M' dense rows, as [n][h'][w'][row_bytes])."""
    n, h, w = shape
    nbytes = n * _sub(h) * _sub(w) * row_bytes
    buf = out_buf(nbytes + TAIL, torch.uint8, POISON)
    conv.out_q, conv.out_sub = buf.data_ptr(), S
    lib.call(entry, C.byref(args), stream())
    conv.out_sub = 0
    got = buf.cpu().numpy()
    assert (got[nbytes:] == POISON).all(), (what, "bytes written behind the M' output rows")
    return got[:nbytes].reshape(n, _sub(h), _sub(w), row_bytes)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("tie", [False, True])
def test_solo_kernel_equals_the_dense_launch_gathered(lib, orc, c, shape, tie):
    n, h, w = shape
    c3 = 4 * c
    a, keep, o = _solo_case(lib, orc, c, shape, tie)
    ex = a.expand
    nvar = lib.load().hawq_conv_expand_reduce_variants(C.byref(a))
    assert nvar >= 1
    ex.out_sub = S
    assert lib.load().hawq_conv_expand_reduce_variants(C.byref(a)) == nvar   # the recorded plans' pair_variant_counts must keep matching
    ex.out_sub = 0
    ft = ex.fast_tables
    mq4, eq4, q4_ref = _nibble_table(orc, o)
    mq8, eq8 = ex.mq, ex.eq
    for bits in (8, 4):
        row_bytes = c3 * bits // 8
        ex.out_bits, ex.q_lo, ex.q_hi = (8, 0, 127) if bits == 8 else (4, 0, 15)
        ex.mq, ex.eq = (mq8, eq8) if bits == 8 else (mq4, eq4)
        # tie-free tables with all per-channel pre-shifts zero (bit 3), the general form, exact ties (force_tie: fast_tables == 5)
        for k0 in (0, 8) if (keep['k0'] and not tie) else (0,):
            ex.fast_tables = ft | k0
            dense = out_buf(n * h * w * row_bytes, torch.uint8, POISON)
            ex.out_q, a.tile = dense.data_ptr(), 0
            lib.call("hawq_conv_expand_reduce", C.byref(a), stream())
            want = _dense_rows(dense, shape, row_bytes)[:, ::S, ::S]
            for tile in range(1, nvar + 1):
                a.tile = tile
                got = _launch_sub(lib, "hawq_conv_expand_reduce", a, ex, shape, row_bytes, (bits, k0, tile))
                assert np.array_equal(got, want), (bits, k0, tile)
                assert keep['flags'].item() == 0
    ex.fast_tables, ex.mq, ex.eq = ft, mq8, eq8


@pytest.mark.parametrize("c", CHANNELS)
def test_solo_kernel_equals_the_oracle(lib, orc, c):
    """One case per channel count straight against the CPU oracle's block input (int8 and hawq4), every variant."""
    shape = SHAPES[CHANNELS.index(c)]
    n, h, w = shape
    c3 = 4 * c
    a, keep, o = _solo_case(lib, orc, c, shape, False)
    ex = a.expand
    mq4, eq4, q4_ref = _nibble_table(orc, o)
    for bits, ref in ((8, keep['q_ref']), (4, q4_ref)):
        if bits == 4:
            ex.out_bits, ex.q_lo, ex.q_hi, ex.mq, ex.eq = 4, 0, 15, mq4, eq4
        for tile in range(1, lib.load().hawq_conv_expand_reduce_variants(C.byref(a)) + 1):
            a.tile = tile
            got = _launch_sub(lib, "hawq_conv_expand_reduce", a, ex, shape, c3 * bits // 8, (bits, tile))
            q = unpack_q(torch.from_numpy(np.ascontiguousarray(got).reshape(-1)), (n, _sub(h), _sub(w), c3), bits)
            assert np.array_equal(q, ref[:, :, ::S, ::S]), (bits, tile)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("res_bits", [16, 32])
@pytest.mark.parametrize("fast", [True, False])
def test_generic_path_equals_the_dense_launch_gathered(lib, orc, c, shape, res_bits, fast):
    """hawq_conv2d with the RESIDUAL epilogue - what the tuner's plain-launch candidate and the int32-residual twin run: fast and
    general tables, uint16 and int32 res_in, every tile id that takes the launch."""
    n, h, w = shape
    c3 = 4 * c
    a, keep, o = _solo_case(lib, orc, c, shape, False)
    ex = a.expand
    if res_bits == 32:
        keep['res32'] = dev(keep['res'].cpu().numpy().astype(np.int32))
        ex.res_in, ex.res_in_bits = keep['res32'].data_ptr(), 32
    if not fast:
        ex.fast_tables = 0
    ref = keep['q_ref'][:, :, ::S, ::S]
    n_tiles, n_special = lib.load().hawq_conv2d_num_tiles(), lib.load().hawq_conv2d_num_band_tiles()
    took = 0
    for tile in range(0, n_tiles + 1):
        ex.tile, ex.out_sub = tile, S
        scratch = out_buf(n * h * w * c3 + TAIL, torch.uint8, None)
        ex.out_q = scratch.data_ptr()
        if lib.load().hawq_conv2d(C.byref(ex), stream()) != 0:
            assert tile > n_tiles - n_special, (tile, "a general tile refused the launch")
            ex.out_sub = 0
            continue
        ex.out_sub = 0
        took += 1
        dense = out_buf(n * h * w * c3, torch.uint8, POISON)
        ex.out_q = dense.data_ptr()
        lib.call("hawq_conv2d", C.byref(ex), stream())
        want = _dense_rows(dense, shape, c3)[:, ::S, ::S]
        got = _launch_sub(lib, "hawq_conv2d", ex, ex, shape, c3, (res_bits, fast, tile))
        assert np.array_equal(got, want), (res_bits, fast, tile)
        q = unpack_q(torch.from_numpy(np.ascontiguousarray(got).reshape(-1)), (n, _sub(h), _sub(w), c3), 8)
        assert np.array_equal(q, ref), (res_bits, fast, tile)
    assert took >= n_tiles - n_special + 1   # the heuristic (0) and every general tile
    ex.tile = 0


def test_everything_else_refuses_out_sub(lib, orc):
    from hawq_amd.packing import pack_w1x1_k128
    L = lib.load()
    n, h, w, c, c3 = 2, 7, 7, 128, 512
    a, keep, o, _ = _case(lib, orc, n, h, w, c, c3, 77)
    ex = a.expand
    # the fused pairs (fused_er.hip, fused_er2.hip, fused_wp.hip with the reduce conv)
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) >= 1
    ex.out_sub = S
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0 and L.hawq_conv_expand_reduce(C.byref(a), None) != 0
    ex.out_sub, a.reduce.out_sub = 0, S
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0
    a.reduce.out_sub = 0
    # the expand conv alone: same count with and without, but not with a dense residual to write
    a.reduce = lib.ExpandReduceArgs().reduce
    qbuf = out_buf(n * h * w * c3, torch.uint8, 0)
    ex.out_q, ex.res_out = qbuf.data_ptr(), None
    nsolo = L.hawq_conv_expand_reduce_variants(C.byref(a))
    ex.out_sub = S
    assert nsolo >= 1 and L.hawq_conv_expand_reduce_variants(C.byref(a)) == nsolo
    ex.res_out = keep['res_out'].data_ptr()
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0 and L.hawq_conv2d(C.byref(ex), None) != 0
    ex.res_out, ex.out_sub = None, 0
    # the streaming 1x1 kernels take the launch without the field and refuse it with it; so does split-K
    keep['wk'] = dev(pack_w1x1_k128(keep['w3'].cpu().numpy(), c3, c))
    ex.wgt_k128 = keep['wk'].data_ptr()
    first, ng2 = L.hawq_conv2d_gemm2_first(), L.hawq_conv2d_num_gemm2_tiles()
    took = 0
    for tile in range(first, first + ng2):
        ex.tile, ex.out_sub = tile, 0
        if L.hawq_conv2d(C.byref(ex), stream()) == 0:
            took += 1
        ex.out_sub = S
        assert L.hawq_conv2d(C.byref(ex), None) != 0, tile
    assert took >= 1
    n_tiles, n_special = L.hawq_conv2d_num_tiles(), L.hawq_conv2d_num_band_tiles()
    for tile in range(n_tiles - n_special + 1, n_tiles + 1):   # band, weight-stationary, band_v2, gemm_v2
        ex.tile = tile
        assert L.hawq_conv2d(C.byref(ex), None) != 0, tile
    ex.tile = 0
    assert L.hawq_conv2d_band_tile(C.byref(ex)) == 0 and L.hawq_conv2d_band2_tile(C.byref(ex)) == 0
    ex.out_sub = 0
    assert L.hawq_conv2d_splitk_ok(C.byref(ex), 2) == 1
    ex.out_sub = S
    assert L.hawq_conv2d_splitk_ok(C.byref(ex), 2) == 0
    # outside its contract the field is an error, not a silently dense launch
    ex.stride = 2
    assert L.hawq_conv2d(C.byref(ex), None) != 0
    torch.cuda.synchronize()
