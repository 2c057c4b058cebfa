"""hawq_conv_args.out_sub on a 3x3 / stride 1 / pad 1 launch (include/hawq_mi355.h): the second conv of a stage's last bottleneck
evaluated only at the pixels (n, 2 y', 2 x') its 1x1 successor is asked for, stored densely.  The strided twins of the round-5 3x3
kernels (band_v2.hip, planar input) and every general tile (NHWC input) take it; every byte must equal the out_sub = 0 launch
gathered at [:, ::2, ::2], the RAW accumulators must equal the CPU oracle's, nothing may be written behind the M' dense rows, and
band_v1, band_persist, gemm_v2 and split-K must refuse the field through their queries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard import guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_kernels import (conv_args, dev, lib, make_conv, odyadic, orc, pack_act, rand_tables, stream,  # noqa: F401
                                    to_planar)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]

S = 2
# (n, h, w): M' = 32, an image boundary inside one wave tile; non-square, M' = 45, a ragged tile; M' = 125, one short of a 128 tile;
# M' = 147, two tiles, the second ragged and spanning images
SHAPES = [(2, 7, 7), (3, 6, 10), (5, 9, 9), (3, 14, 14)]
CHANNELS = [(64, 64), (128, 128), (256, 64)]
POISON, TAIL = 0xAB, 4096


def _sub(n):
    return (n - 1) // S + 1


def _ids(L):
    """(general tile ids, band_v2 tile ids, every other special-purpose id)."""
    n, nsp, nb2, ng2 = L.hawq_conv2d_num_tiles(), L.hawq_conv2d_num_band_tiles(), L.hawq_conv2d_num_band2_tiles(), L.hawq_conv2d_num_gemm2_tiles()
    general = list(range(1, n - nsp + 1))
    band2 = list(range(n - ng2 - nb2 + 1, n - ng2 + 1))
    return general, band2, [t for t in range(n - nsp + 1, n + 1) if t not in band2]


def _setup(lib, orc, shape, cin, cout, bits, seed, tie=False):
    """A 3x3 conv on random operands: NHWC and planar input, packed weight stream, oracle accumulators, and either provably tie-free
    tables or - `tie` - forced-tie ones as tests/test_gpu_kernels.py::test_conv_requant_epilogue draws them: ratio 1/4 on channel 0
    and 3/16 on channel 1, their accumulators centred on zero, with exact .5 ties AT THE PIXELS (2y, 2x) the strided launch evaluates."""
    from hawq_amd.packing import pack_conv_weight, pack_ctab, pack_w3x3_band
    from hawq_amd.quant_utils import tables_are_fast, tables_fit_fast
    n, h, w = shape
    for attempt in range(8):   # (a map of 32 evaluated pixels may hold no tie on channel 0: draw again, deterministically)
        rng = np.random.default_rng(seed + 7919 * attempt)
        x, wt, b = make_conv(rng, n, h, w, cin, cout, 3, bits, bits)
        acc = orc.conv2d(x, wt, b, 1, 1)
        m, e = rand_tables(rng, cout, 2e-5 if bits == 8 else 2e-3, 3e-4 if bits == 8 else 2e-2)
        if not tie:
            break
        for c in (0, 1):
            b[c] += 2 - int(np.median(acc[:, c]))
        acc = orc.conv2d(x, wt, b, 1, 1)
        m[0], e[0] = 1 << 30, 33 | (1 << 8)   # ratio 1/4 (e = 32 lifted by k = 1): a tie whenever acc = 2 mod 4
        m[1], e[1] = 3 << 29, 34              # ratio 3/16: a tie whenever acc = 8 mod 16
        v0, v1 = acc[:, 0, ::S, ::S].astype(np.int64), acc[:, 1, ::S, ::S].astype(np.int64)
        if ((v0 > 0) & (v0 % 4 == 2)).any() and ((v1 > 0) & (v1 % 16 == 8)).any():
            break
    vbits = int(np.abs(acc).max()).bit_length() + 1
    if tie:
        v0, v1 = acc[:, 0, ::S, ::S].astype(np.int64), acc[:, 1, ::S, ::S].astype(np.int64)
        assert ((v0 > 0) & (v0 % 4 == 2)).any() and ((v1 > 0) & (v1 % 16 == 8)).any()   # the evaluated pixels do hold exact ties
        assert tables_fit_fast(m, e, vbits) and not tables_are_fast(m, e, vbits)
    else:
        assert tables_are_fast(m, e, vbits)
    a, keep = conv_args(lib, x, wt, b, 1, 1, bits, bits)
    keep.update(wb=dev(pack_w3x3_band(pack_conv_weight(wt, bits), cout, cin * bits // 8)), xp=dev(to_planar(pack_act(x, bits))),
                ctab=dev(pack_ctab(b, m, e)), m=dev(m), e=dev(e))
    a.wgt_band = keep['wb'].data_ptr()
    a.m, a.e, a.ctab = keep['m'].data_ptr(), keep['e'].data_ptr(), keep['ctab'].data_ptr()
    return a, keep, acc


def _set_input(a, keep, planar):
    a.in_, a.in_planar = (keep['xp'] if planar else keep['x']).data_ptr(), int(planar)


def _band2_should_take(a):
    """Row of at least two 64-byte slices; the maps of this file are narrow enough for every band."""
    return a.Cin * a.in_bits // 8 >= 128


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("chan", CHANNELS)
def test_every_taker_equals_the_dense_launch_gathered(lib, orc, shape, chan):
    L = lib.load()
    n, h, w = shape
    cin, cout = chan
    general, band2, _ = _ids(L)
    assert len(general) == 15 and len(band2) == 2
    m_out = n * _sub(h) * _sub(w)
    for bits, tie in [(bb, t) for bb in ((8, 4) if cin % 128 == 0 else (8,)) for t in (False, True)]:
        a, keep, acc = _setup(lib, orc, shape, cin, cout, bits, 1000 * h + 10 * w + cin + bits, tie)
        a.epilogue, a.relu = lib.EPI_REQUANT, 1
        dense = out_buf(n * h * w * cout, torch.uint8, POISON)
        sub = out_buf(m_out * cout + TAIL, torch.uint8, POISON)
        for out_bits, (lo, hi) in ((8, (-128, 127)), (4, (0, 15))):
            row = cout * out_bits // 8
            a.out_bits, a.q_lo, a.q_hi = out_bits, lo, hi
            # tie-free tables: the tie-free kernels, and the exact-tie ones on the same tables; forced-tie tables (exact .5 ties at the
            # evaluated pixels): the exact-tie kernels (5), and the exact general kernels (0) on the general tiles
            for mode in (5, 0) if tie else (1, 5):
                a.fast_tables = mode
                _set_input(a, keep, False)
                a.tile, a.out_sub, a.out_q = 0, 0, dense.data_ptr()
                lib.call("hawq_conv2d", C.byref(a), stream())
                want = dense.cpu().numpy()[:n * h * w * row].reshape(n, h, w, row)[:, ::S, ::S]
                if out_bits == 8:   # the dense launch itself is what the oracle says, ties included (the anchor of every mode)
                    ref = odyadic(orc, np.maximum(acc, 0), keep['m'].cpu().numpy(), keep['e'].cpu().numpy(), (lo, hi))
                    assert np.array_equal(want.view(np.int8).astype(np.int64), ref.transpose(0, 2, 3, 1)[:, ::S, ::S])
                a.out_sub, a.out_q = S, sub.data_ptr()
                took = 0
                for tile in general + band2:
                    planar = tile in band2
                    _set_input(a, keep, planar)
                    a.tile = tile
                    if planar and (mode == 0 or not _band2_should_take(a)):   # (the band kernels are fast-contract kernels)
                        assert L.hawq_conv2d(C.byref(a), None) != 0, (tile, "refused, not mis-computed")
                        continue
                    sub.fill_(POISON)
                    lib.call("hawq_conv2d", C.byref(a), stream())
                    got = sub.cpu().numpy()
                    assert (got[m_out * row:] == POISON).all(), (bits, out_bits, mode, tile, "bytes written behind the M' output rows")
                    assert np.array_equal(got[:m_out * row].reshape(n, _sub(h), _sub(w), row), want), (bits, tie, out_bits, mode, tile)
                    took += 1
                assert took == len(general) + (len(band2) if (mode and _band2_should_take(a)) else 0)
                a.out_sub = 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("chan", CHANNELS)
def test_raw_accumulators_equal_the_oracle_gathered(lib, orc, shape, chan):
    L = lib.load()
    n, h, w = shape
    cin, cout = chan
    general, band2, _ = _ids(L)
    m_out = n * _sub(h) * _sub(w)
    for bits in (8, 4) if cin % 128 == 0 else (8,):
        a, keep, acc = _setup(lib, orc, shape, cin, cout, bits, 77 * h + w + cin + bits)
        want = np.ascontiguousarray(acc.transpose(0, 2, 3, 1)[:, ::S, ::S])
        out = out_buf(m_out * cout + TAIL // 4, torch.int32, -7)
        a.epilogue, a.out_acc, a.out_sub = lib.EPI_RAW, out.data_ptr(), S
        for fast in (0, 1):
            a.fast_tables = fast
            for tile in general + (band2 if fast else []):
                planar = tile in band2
                _set_input(a, keep, planar)
                a.tile = tile
                if planar and not _band2_should_take(a):
                    assert L.hawq_conv2d(C.byref(a), None) != 0
                    continue
                out.fill_(-7)
                lib.call("hawq_conv2d", C.byref(a), stream())
                got = out.cpu().numpy()
                assert (got[m_out * cout:] == -7).all(), (bits, tile, "words written behind the M' output rows")
                assert np.array_equal(got[:m_out * cout].reshape(want.shape), want), (bits, fast, tile)


def test_everything_else_refuses_the_strided_3x3(lib, orc):
    L = lib.load()
    general, band2, others = _ids(L)
    # Cin = Cout = 64 on a 14 x 14 map: band_v1 and the weight-stationary kernel take the dense launch
    a, keep, acc = _setup(lib, orc, (2, 14, 14), 64, 64, 8, 5)
    out = out_buf(2 * 14 * 14 * 64, torch.uint8, 0)
    a.epilogue, a.relu, a.fast_tables = lib.EPI_REQUANT, 1, 1
    a.out_q, a.out_bits, a.q_lo, a.q_hi = out.data_ptr(), 8, -128, 127
    ch = lib.ConvChoice()
    dense_takers = []
    for planar in (False, True):
        _set_input(a, keep, planar)
        for tile in others:
            a.tile, a.out_sub = tile, 0
            if L.hawq_conv2d_choice(C.byref(a), C.byref(ch)) == 0:
                dense_takers.append(tile)
            a.out_sub = S
            assert L.hawq_conv2d_choice(C.byref(a), C.byref(ch)) != 0 and L.hawq_conv2d(C.byref(a), None) != 0, (tile, planar)
    assert len(set(dense_takers)) >= 2   # a band_v1 id and a weight-stationary id at least
    a.tile = 0
    _set_input(a, keep, False)
    a.out_sub = 0
    assert L.hawq_conv2d_band_tile(C.byref(a)) != 0
    a.out_sub = S
    assert L.hawq_conv2d_band_tile(C.byref(a)) == 0
    # split-K takes the dense 3x3 and refuses the strided one
    a.out_sub = 0
    assert L.hawq_conv2d_splitk_ok(C.byref(a), 3) == 1
    a.out_sub = S
    assert L.hawq_conv2d_splitk_ok(C.byref(a), 3) == 0
    # no planar output
    a.out_planar = 1
    assert L.hawq_conv2d(C.byref(a), None) != 0
    a.out_planar = 0
    assert L.hawq_conv2d_choice(C.byref(a), C.byref(ch)) == 0 and ch.res_sub == 0 and ch.stride == S and (ch.Ho, ch.Wo, ch.M) == (7, 7, 98)
    torch.cuda.synchronize()


def test_a_map_too_wide_for_the_band_runs_on_a_general_tile(lib, orc):
    """(1, 8, 250): 128 outputs span two source rows of 250 pixels and the rows around them, 64 outputs one - neither fits its band
    (a 120-wide map still does: 744 of 764 and 496 of 508 band pixels).  The query says 0 (the engine then keeps NHWC rows) and the
    general tiles still compute the launch."""
    L = lib.load()
    shape, cin, cout = (1, 8, 250), 128, 64
    n, h, w = shape
    a, keep, acc = _setup(lib, orc, shape, cin, cout, 8, 9)
    a.epilogue, a.relu, a.fast_tables = lib.EPI_REQUANT, 1, 1
    a.out_bits, a.q_lo, a.q_hi = 8, -128, 127
    m_out = n * _sub(h) * _sub(w)
    sub = out_buf(m_out * cout + TAIL, torch.uint8, POISON)
    a.out_q = sub.data_ptr()
    _set_input(a, keep, True)
    a.out_sub = 0
    assert L.hawq_conv2d_band2_tile(C.byref(a)) == 0   # (even the dense launch: a 250-wide map)
    a.out_sub = S
    ext = (C.c_int32 * 5)()
    for index in range(L.hawq_conv2d_num_band2_tiles()):
        worst = 0
        assert L.hawq_conv2d_band2_sub_extent(C.byref(a), index, 0, ext) == 0
        for t in range(ext[3]):
            assert L.hawq_conv2d_band2_sub_extent(C.byref(a), index, t, ext) == 0
            worst = max(worst, ext[1])
        assert worst > ext[2] - 4, (index, worst, ext[2])
    assert L.hawq_conv2d_band2_tile(C.byref(a)) == 0
    for tile in _ids(L)[1]:
        a.tile = tile
        assert L.hawq_conv2d(C.byref(a), None) != 0
    _set_input(a, keep, False)
    a.tile = 0
    lib.call("hawq_conv2d", C.byref(a), stream())
    got = sub.cpu().numpy()
    assert (got[m_out * cout:] == POISON).all()
    ref = odyadic(orc, np.maximum(acc, 0), keep['m'].cpu().numpy(), keep['e'].cpu().numpy(), (-128, 127))
    assert np.array_equal(got[:m_out * cout].view(np.int8).astype(np.int64).reshape(n, _sub(h), _sub(w), cout), ref.transpose(0, 2, 3, 1)[:, ::S, ::S])


@pytest.mark.parametrize("tie", [False, True])
def test_a_band_four_pixels_short_of_its_stage(lib, orc, tie):
    """(1, 8, 120), what the band can just hold: 744 of the 764 usable band pixels of the 128-output twin, 496 of 508 of the 64-output
    one - the last 64-pixel group of every plane is filled and its four masked lanes sit right behind the data.  Both twins against
    the dense launch (a general tile: the dense band kernels refuse a 120-wide map) gathered, and against the oracle."""
    L = lib.load()
    shape, cin, cout = (1, 8, 120), 128, 64
    n, h, w = shape
    general, band2, _ = _ids(L)
    a, keep, acc = _setup(lib, orc, shape, cin, cout, 8, 120, tie)
    a.epilogue, a.relu, a.fast_tables = lib.EPI_REQUANT, 1, 5 if tie else 1
    a.out_bits, a.q_lo, a.q_hi = 8, -128, 127
    m_out = n * _sub(h) * _sub(w)
    dense = out_buf(n * h * w * cout, torch.uint8, POISON)
    sub = out_buf(m_out * cout + TAIL, torch.uint8, POISON)
    _set_input(a, keep, False)
    a.tile, a.out_sub, a.out_q = 0, 0, dense.data_ptr()
    lib.call("hawq_conv2d", C.byref(a), stream())
    want = dense.cpu().numpy().reshape(n, h, w, cout)[:, ::S, ::S]
    ref = odyadic(orc, np.maximum(acc, 0), keep['m'].cpu().numpy(), keep['e'].cpu().numpy(), (-128, 127))
    assert np.array_equal(want.view(np.int8).astype(np.int64), ref.transpose(0, 2, 3, 1)[:, ::S, ::S])
    a.out_sub, a.out_q = S, sub.data_ptr()
    _set_input(a, keep, True)
    ext = (C.c_int32 * 5)()
    for index, tile in enumerate(band2):
        worst = 0
        assert L.hawq_conv2d_band2_sub_extent(C.byref(a), index, 0, ext) == 0
        for t in range(ext[3]):
            assert L.hawq_conv2d_band2_sub_extent(C.byref(a), index, t, ext) == 0
            worst = max(worst, ext[1])
        assert ext[2] - 64 < worst <= ext[2] - 4, (index, worst, ext[2])   # reaches into the last 64-pixel group, and fits
        a.tile = tile
        sub.fill_(POISON)
        lib.call("hawq_conv2d", C.byref(a), stream())
        got = sub.cpu().numpy()
        assert (got[m_out * cout:] == POISON).all(), tile
        assert np.array_equal(got[:m_out * cout].reshape(n, _sub(h), _sub(w), cout), want), tile
