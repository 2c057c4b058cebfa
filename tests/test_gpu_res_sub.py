""""res_sub" (hawq_conv_args.H2 / W2 / stride2 of a single-branch RESIDUAL launch, include/hawq_mi355.h): the expand conv behind a 3x3 launch that ran with out_sub.  `in` and out_q are dense
over the small [N][H'][W'] grid, only res_in still lives on the full map and is read at (n, s y, s x).  A res_sub launch on
x2[:, ::2, ::2] made contiguous must equal, byte for byte, the out_sub launch on the full map - for the solo variants of the
wave-private kernel (fused_wp.hip) and for hawq_conv2d's general tiles; the variant counts must not move with the field set and the
fused pairs must refuse it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard import guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_fused import _case
from tests.test_gpu_kernels import dev, lib, orc, stream, unpack_q  # noqa: F401
from tests.test_gpu_out_sub import CHANNELS, POISON, S, SHAPES, TAIL, _launch_sub, _nibble_table, _solo_case, _sub

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]


def _small_input(keep, shape, c):
    """x2[:, ::S, ::S] of the case's NHWC input, contiguous, on the device."""
    n, h, w = shape
    x = keep['x2'].cpu().numpy().reshape(n, h, w, c)
    return dev(np.ascontiguousarray(x[:, ::S, ::S]))


def _launch_res_sub(lib, entry, args, conv, keep, shape, row_bytes, what):
    """Launch `entry` with `conv` turned into the res_sub form (dense small-map input, residual on the full map) into a poisoned
    buffer; the struct is restored.  Returns the M' dense rows as [n][h'][w'][row_bytes]."""
    n, h, w = shape
    nbytes = n * _sub(h) * _sub(w) * row_bytes
    buf = out_buf(nbytes + TAIL, torch.uint8, POISON)
    full_in = conv.in_
    conv.in_, conv.H, conv.W = keep['x2s'].data_ptr(), _sub(h), _sub(w)
    conv.stride2, conv.H2, conv.W2, conv.out_q = S, h, w, buf.data_ptr()
    try:
        lib.call(entry, C.byref(args), stream())
    finally:
        conv.in_, conv.H, conv.W = full_in, h, w
        conv.stride2 = conv.H2 = conv.W2 = 0
    got = buf.cpu().numpy()
    assert (got[nbytes:] == POISON).all(), (what, "bytes written behind the M' output rows")
    return got[:nbytes].reshape(n, _sub(h), _sub(w), row_bytes)


def _as_res_sub(conv, keep, shape):
    n, h, w = shape
    conv.in_, conv.H, conv.W = keep['x2s'].data_ptr(), _sub(h), _sub(w)
    conv.stride2, conv.H2, conv.W2 = S, h, w


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("tie", [False, True])
def test_solo_kernel_equals_the_out_sub_launch(lib, orc, c, shape, tie):
    c3 = 4 * c
    a, keep, o = _solo_case(lib, orc, c, shape, tie)
    keep['x2s'] = _small_input(keep, shape, c)
    ex = a.expand
    nvar = lib.load().hawq_conv_expand_reduce_variants(C.byref(a))
    assert nvar >= 1
    full_in = ex.in_
    _as_res_sub(ex, keep, shape)
    assert lib.load().hawq_conv_expand_reduce_variants(C.byref(a)) == nvar   # the recorded plans' pair_variant_counts must keep matching
    ex.in_, ex.H, ex.W, ex.stride2, ex.H2, ex.W2 = full_in, shape[1], shape[2], 0, 0, 0
    mq4, eq4, _ = _nibble_table(orc, o)
    mq8, eq8 = ex.mq, ex.eq
    for bits in (8, 4):
        row_bytes = c3 * bits // 8
        ex.out_bits, ex.q_lo, ex.q_hi = (8, 0, 127) if bits == 8 else (4, 0, 15)
        ex.mq, ex.eq = (mq8, eq8) if bits == 8 else (mq4, eq4)
        a.tile = 0
        want = _launch_sub(lib, "hawq_conv_expand_reduce", a, ex, shape, row_bytes, (bits, "out_sub"))
        for tile in range(1, nvar + 1):
            a.tile = tile
            got = _launch_res_sub(lib, "hawq_conv_expand_reduce", a, ex, keep, shape, row_bytes, (bits, tile))
            assert np.array_equal(got, want), (bits, tile)
            assert keep['flags'].item() == 0
    ex.mq, ex.eq = mq8, eq8


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("res_bits", [16, 32])
@pytest.mark.parametrize("fast", [True, False])
def test_general_tiles_equal_the_out_sub_launch(lib, orc, c, shape, res_bits, fast):
    L = lib.load()
    c3 = 4 * c
    a, keep, o = _solo_case(lib, orc, c, shape, False)
    keep['x2s'] = _small_input(keep, shape, c)
    ex = a.expand
    if res_bits == 32:
        keep['res32'] = dev(keep['res'].cpu().numpy().astype(np.int32))
        ex.res_in, ex.res_in_bits = keep['res32'].data_ptr(), 32
    if not fast:
        ex.fast_tables = 0
    mq4, eq4, _ = _nibble_table(orc, o)
    mq8, eq8 = ex.mq, ex.eq
    n_tiles, n_special = L.hawq_conv2d_num_tiles(), L.hawq_conv2d_num_band_tiles()
    for bits in (8, 4):
        row_bytes = c3 * bits // 8
        ex.out_bits, ex.q_lo, ex.q_hi = (8, 0, 127) if bits == 8 else (4, 0, 15)
        ex.mq, ex.eq = (mq8, eq8) if bits == 8 else (mq4, eq4)
        ex.tile = 0
        want = _launch_sub(lib, "hawq_conv2d", ex, ex, shape, row_bytes, (bits, "out_sub"))
        for tile in range(0, n_tiles - n_special + 1):   # the heuristic and every general tile
            ex.tile = tile
            got = _launch_res_sub(lib, "hawq_conv2d", ex, ex, keep, shape, row_bytes, (res_bits, fast, bits, tile))
            assert np.array_equal(got, want), (res_bits, fast, bits, tile)
    ex.tile, ex.mq, ex.eq = 0, mq8, eq8


@pytest.mark.parametrize("c", CHANNELS)
def test_res_sub_equals_the_oracle(lib, orc, c):
    """One case per channel count straight against the CPU oracle's block input: every solo variant and the heuristic general tile."""
    shape = SHAPES[CHANNELS.index(c)]
    n, h, w = shape
    c3 = 4 * c
    a, keep, o = _solo_case(lib, orc, c, shape, False)
    keep['x2s'] = _small_input(keep, shape, c)
    ex = a.expand
    ref = keep['q_ref'][:, :, ::S, ::S]
    for tile in range(1, lib.load().hawq_conv_expand_reduce_variants(C.byref(a)) + 1):
        a.tile = tile
        got = _launch_res_sub(lib, "hawq_conv_expand_reduce", a, ex, keep, shape, c3, ("solo", tile))
        q = unpack_q(torch.from_numpy(np.ascontiguousarray(got).reshape(-1)), (n, _sub(h), _sub(w), c3), 8)
        assert np.array_equal(q, ref), tile
    ex.tile = 0
    got = _launch_res_sub(lib, "hawq_conv2d", ex, ex, keep, shape, c3, "general")
    q = unpack_q(torch.from_numpy(np.ascontiguousarray(got).reshape(-1)), (n, _sub(h), _sub(w), c3), 8)
    assert np.array_equal(q, ref)


def test_everything_else_refuses_res_sub(lib, orc):
    from hawq_amd.packing import pack_w1x1_k128
    L = lib.load()
    shape = (2, 7, 7)
    n, h, w = shape
    c, c3 = 128, 512
    a, keep, o, _ = _case(lib, orc, n, h, w, c, c3, 77)
    keep['x2s'] = _small_input(keep, shape, c)
    ex = a.expand
    full = (ex.in_, ex.H, ex.W)

    def restore():
        ex.in_, ex.H, ex.W = full
        ex.stride2 = ex.H2 = ex.W2 = 0
    # the fused pairs (fused_er.hip, fused_er2.hip, fused_wp.hip with the reduce conv)
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) >= 1
    a.reduce.H, a.reduce.W = _sub(h), _sub(w)
    _as_res_sub(ex, keep, shape)
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0 and L.hawq_conv_expand_reduce(C.byref(a), None) != 0
    restore()
    a.reduce.H, a.reduce.W = h, w
    # the expand conv alone: same count with and without, but not with a dense residual to write, not together with out_sub, and not
    # on a residual map of another size
    a.reduce = lib.ExpandReduceArgs().reduce
    qbuf = out_buf(n * h * w * c3, torch.uint8, 0)
    ex.out_q, ex.res_out = qbuf.data_ptr(), None
    nsolo = L.hawq_conv_expand_reduce_variants(C.byref(a))
    _as_res_sub(ex, keep, shape)
    assert nsolo >= 1 and L.hawq_conv_expand_reduce_variants(C.byref(a)) == nsolo
    ex.res_out = keep['res_out'].data_ptr()
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0 and L.hawq_conv2d(C.byref(ex), None) != 0
    ex.res_out, ex.out_sub = None, S
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0 and L.hawq_conv2d(C.byref(ex), None) != 0
    ex.out_sub, ex.H2 = 0, h + 2
    assert L.hawq_conv_expand_reduce_variants(C.byref(a)) == 0 and L.hawq_conv2d(C.byref(ex), None) != 0
    ex.H2 = h
    # the streaming 1x1 kernels and split-K take the small dense launch without the field and refuse it with it
    keep['wk'] = dev(pack_w1x1_k128(keep['w3'].cpu().numpy(), c3, c))
    ex.wgt_k128 = keep['wk'].data_ptr()
    keep['res_s'] = dev(np.ascontiguousarray(keep['res'].cpu().numpy().reshape(n, h, w, c3)[:, ::S, ::S]))
    full_res = ex.res_in
    first, ng2 = L.hawq_conv2d_gemm2_first(), L.hawq_conv2d_num_gemm2_tiles()
    ch = lib.ConvChoice()
    took = 0
    for tile in range(first, first + ng2):
        ex.tile = tile
        ex.stride2, ex.res_in = 0, keep['res_s'].data_ptr()
        took += int(L.hawq_conv2d_choice(C.byref(ex), C.byref(ch)) == 0)
        ex.stride2, ex.res_in = S, full_res
        assert L.hawq_conv2d_choice(C.byref(ex), C.byref(ch)) != 0 and L.hawq_conv2d(C.byref(ex), None) != 0, tile
    assert took >= 1
    n_tiles, n_special = L.hawq_conv2d_num_tiles(), L.hawq_conv2d_num_band_tiles()
    for tile in range(n_tiles - n_special + 1, n_tiles + 1):   # band, weight-stationary, band_v2, gemm_v2
        ex.tile = tile
        assert L.hawq_conv2d(C.byref(ex), None) != 0, tile
    ex.tile = 0
    assert L.hawq_conv2d_choice(C.byref(ex), C.byref(ch)) == 0 and ch.res_sub == S and ch.stride == 1 and (ch.Ho, ch.Wo) == (_sub(h), _sub(w))
    ex.stride2 = 0
    assert L.hawq_conv2d_splitk_ok(C.byref(ex), 2) == 1
    ex.stride2 = S
    assert L.hawq_conv2d_splitk_ok(C.byref(ex), 2) == 0
    # outside its contract the field is an error, not a silently dense launch
    ex.stride = 2
    assert L.hawq_conv2d(C.byref(ex), None) != 0
    torch.cuda.synchronize()
