"""Every kernel on the last shape its check accepts (tests/contract_edges.py: the capacity rules restated, the run-ends and their
first refused neighbours): an LDS band exactly full, a map one pixel wide, a second column chunk, the largest map of a tile family,
a sum at the edge of int32, a pixel index just under 2^23.  Bit-exact against the oracle through the case builders of the kernel
families' own test files; every buffer of every case comes from the guard arena.  Each case asserts from its shape that it reaches
the seam it is named for (tile count, image straddle, chunk count, band slack), so it cannot silently degenerate."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import tests.test_gpu_band2 as B2
import tests.test_gpu_conv2_sub as CS
import tests.test_gpu_incep_stem_f32 as ST
import tests.test_gpu_kernels as K
from tests import contract_edges as CE
from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.requant_corners import clamp, rne
from tests.test_gpu_kernels import lib, orc  # noqa: F401  (fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]

CHANNELS = [(64, 64), (128, 128), (256, 128)]


def _reaches_the_seams(n, h, w, bms):
    """at least two full pixel tiles and a ragged one, and a tile across the boundary between the two images"""
    assert n == 2
    for bm in bms:
        m = n * h * w
        assert m // bm >= 2 and m % bm != 0, (m, bm)
        assert (h * w) % bm != 0, (h * w, bm)   # the tile that holds the last pixel of image 0 also holds the first of image 1


# ------------------------------------------------------------------ a. band_v1 and the weight-stationary kernel
def _ends_here(w, chan, bits):
    """the tiles that take the layer and have a run that begins or ends at this width"""
    return [i for i in CE.band_takers(w, chan[0], chan[1], bits) if w in CE.run_ends(CE.BAND_RUNS[CE.BAND_TILES[i].name])]


def _band_case(w, chan, bits):
    cin, cout = chan
    takers = CE.band_takers(w, cin, cout, bits)
    h = CE.band_seam_height(w)
    _reaches_the_seams(2, h, w, {CE.BAND_TILES[i].bm for i in takers})
    # the width is a run-end of a tile that runs here, and an upper end leaves at most eight band pixels unused
    ends = _ends_here(w, chan, bits)
    assert ends, (w, chan, bits)
    for i in ends:
        t = CE.BAND_TILES[i]
        if any(b == w for _, b in CE.BAND_RUNS[t.name]):
            assert 0 <= CE.band_slack(t, w) <= 8, (t.name, w)
    return (2, h, w, cin, cout), takers


# every width at which a run of some tile ends, at the channel counts and operand widths at which such a tile takes the layer
BAND_CASES = [(w, chan, bits) for w in CE.BAND_WIDTHS for chan in CHANNELS for bits in (8, 4)
              if (bits == 8 or chan[0] % 128 == 0) and _ends_here(w, chan, bits)]


@pytest.mark.parametrize("w,chan,bits", BAND_CASES)
def test_band_run_ends_requant(lib, orc, w, chan, bits):
    shape, takers = _band_case(w, chan, bits)
    assert takers
    K.test_conv3x3_band_kernels(lib, orc, shape, bits, expect=takers)


@pytest.mark.parametrize("w,chan,bits", BAND_CASES)
@pytest.mark.parametrize("mode", [1, 5])
def test_band_run_ends_residual(lib, orc, w, chan, bits, mode):
    shape, takers = _band_case(w, chan, bits)
    K.test_conv3x3_band_residual(lib, orc, shape, bits, mode, expect=takers)


def test_every_run_end_of_every_tile_is_launched():
    for i, t in enumerate(CE.BAND_TILES):
        for w in CE.run_ends(CE.BAND_RUNS[t.name]):
            assert any(i in CE.band_takers(cw, *chan, bits) for cw, chan, bits in BAND_CASES if cw == w), (t.name, w)


@pytest.mark.parametrize("w", CE.BAND_REFUSED_WIDTHS)
def test_band_first_refused_widths_are_errors(lib, orc, w):
    """hawq_conv2d on every band tile at the first width past each of its runs: non-zero, and nothing written"""
    from hawq_amd.packing import pack_ctab
    first = lib.load().hawq_conv2d_num_tiles() - lib.load().hawq_conv2d_num_band_tiles() + 1
    asked = 0
    for chan in CHANNELS:
        cin, cout = chan
        rng = np.random.default_rng(w + cin)
        x, wt, b = K.make_conv(rng, 2, 4, w, cin, cout, 3, 8, 8)
        m, e = K.rand_tables(rng, cout, 2e-5, 3e-4)
        a, keep = K.conv_args(lib, x, wt, b, 1, 1, 8, 8)
        keep.update(ctab=dev(pack_ctab(b, m, e)), m=dev(m), e=dev(e))
        out = out_buf(2 * 4 * w * cout, torch.uint8, 0x3C)
        a.epilogue, a.relu, a.m, a.e, a.ctab, a.fast_tables = lib.EPI_REQUANT, 1, keep['m'].data_ptr(), keep['e'].data_ptr(), keep['ctab'].data_ptr(), 1
        a.out_q, a.out_bits, a.q_lo, a.q_hi = out.data_ptr(), 8, -128, 127
        for i, t in enumerate(CE.BAND_TILES):
            name = {"B1": "B0", "WS1": "B0", "WS2": "B0", "B4": "B2", "B5": "B2"}.get(t.name, t.name)
            if w not in CE.BAND_REFUSED[name]:
                continue
            assert i not in CE.band_takers(w, cin, cout)
            a.tile = first + i
            assert lib.load().hawq_conv2d(C.byref(a), None) != 0, (t.name, w, chan)
            asked += 1
        assert (out == 0x3C).all()
    assert asked >= 3


# ------------------------------------------------------------------ b. band_v2
BAND2_WIDTHS = [1, 2, 57]


def _band2_shape(w, cin, cout):
    h = CE.seam_height(w)
    _reaches_the_seams(2, h, w, {t.bm for t in CE.BAND2_TILES})
    assert all(CE.band2_fits(t, w) for t in CE.BAND2_TILES)
    if w == 57:
        assert all(t.band_px - 4 - CE.band2_used(t.bm, w) == 1 for t in CE.BAND2_TILES)   # one pixel short of the stage
    return (2, h, w, cin, cout)


@pytest.mark.parametrize("w", BAND2_WIDTHS)
@pytest.mark.parametrize("mode", [1, 5])
def test_band2_run_ends_requant_and_residual(lib, orc, w, mode):
    B2.test_band2_requant(lib, orc, _band2_shape(w, 128, 128), mode)
    B2.test_band2_residual(lib, orc, _band2_shape(w, 192, 64), mode)


@pytest.mark.parametrize("w", BAND2_WIDTHS)
def test_band2_run_ends_hawq4_and_raw(lib, orc, w):
    B2.test_band2_hawq4_operands_and_outputs(lib, orc, _band2_shape(w, 256, 64), 1)
    for bits in (8, 4):
        B2.test_band2_raw_accumulators(lib, orc, _band2_shape(w, 256, 64), bits)


def test_band2_refuses_a_58_wide_map(lib, orc):
    w = 58
    assert not any(CE.band2_fits(t, w) for t in CE.BAND2_TILES)
    rng = np.random.default_rng(w)
    x, wt, b = K.make_conv(rng, 2, 3, w, 128, 64, 3, 8, 8)
    for tile in B2._ids(lib):
        a, keep = B2._args(lib, x, wt, b, tile)
        out = out_buf(2 * 3 * w * 64, torch.int32, -7)
        a.epilogue, a.out_acc = lib.EPI_RAW, out.data_ptr()
        assert lib.load().hawq_conv2d(C.byref(a), None) != 0, tile
        assert (out == -7).all()


@pytest.mark.parametrize("chan", [(128, 128), (256, 64)])
def test_strided_twins_at_their_widest_source_width(lib, orc, chan):
    w = CE.SUB_WIDEST["V128"]
    assert w == CE.SUB_WIDEST["V256"]   # both twins end at the same width on this map, so one shape runs both
    shape = (CE.SUB_N, CE.SUB_H, w)
    ext = (C.c_int32 * 5)()
    a, keep, _ = CS._setup(lib, orc, shape, chan[0], chan[1], 8, 3)
    a.out_sub, a.in_planar = 2, 1
    for index, t in enumerate(CE.BAND2_TILES):
        assert CE.band2_sub_fits(t, *shape) and not CE.band2_sub_fits(t, CE.SUB_N, CE.SUB_H, w + 1)
        # (64 output columns: the launch is whole tiles, five of 128 or ten of 64 outputs; the twins' ragged tiles are tests/test_gpu_conv2_sub.py's)
        assert lib.load().hawq_conv2d_band2_sub_extent(C.byref(a), index, 0, ext) == 0 and ext[3] >= 3
    CS.test_every_taker_equals_the_dense_launch_gathered(lib, orc, shape, chan)
    CS.test_raw_accumulators_equal_the_oracle_gathered(lib, orc, shape, chan)


# ------------------------------------------------------------------ c. incep_stem_f32 column chunks
@pytest.mark.parametrize("shape", sorted(CE.STEM_SHAPES), ids=lambda s: "{}x{}x{}".format(*s))
@pytest.mark.parametrize("channels", ST.CHANNELS, ids=lambda c: "c{}_ldo{}_off{}".format(*c))
def test_stem_f32_column_chunks(shape, channels):
    """(1, 11, 319) is the last width with ONE chunk, exactly full; every other shape has a chunk > 0, the last one 1, 2 or 159 wide"""
    cout, ldo, c_off = channels
    wo, nchunks, last = CE.stem_chunks(shape[2])
    assert (nchunks, last) == CE.STEM_SHAPES[shape]
    assert nchunks >= 2 or (wo == CE.STEM_CW and shape[2] == 319)
    x, inv, in_lo, in_hi, w, b, m, ek, acc = ST._operands(shape, cout)
    assert acc.shape[2] == wo
    for relu, qrange in ((1, (-128, 127)), (0, (-128, 127)), (1, (0, 15)), (0, (0, 15))):
        v, want = ST._expected(acc, b, m, ek, relu, qrange)
        got, base = ST._run_both(x, inv, in_lo, in_hi, w, b, m, ek, cout, ldo, c_off, relu, qrange)
        ST._check(got, base, want, cout, c_off)
        assert len(np.unique(want[:, :, -last:])) > 4   # the last chunk's columns are not all alike


# ------------------------------------------------------------------ d. wide bottleneck units
def test_wide_units_on_8_by_8_are_cases_of_the_unit_test():
    import tests.test_gpu_mbv2_kernels as MB
    for u in CE.LB_WIDE_UNITS:
        assert u in MB.UNITS


@pytest.mark.parametrize("cin,cout,stride,hw", CE.LB_WIDE_REFUSED)
def test_wide_units_refuse_a_ninth_row_or_column(lib, cin, cout, stride, hw):
    n, (h, w) = 2, hw
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    big = out_buf(1 << 20, torch.int32, 7)   # every operand pointer: the launch must refuse before it reads or writes anything
    assert n * h * w * 192 + 320 * 960 < big.numel() * 4
    b = CE.bottleneck_args(cin, cout, stride, (n, h, w), ptr=big.data_ptr())
    assert lib.load().hawq_linear_bottleneck_ok(C.byref(b)) == 0
    assert lib.load().hawq_linear_bottleneck(C.byref(b), None) != 0 and "8 x 8" in lib.load().hawq_last_error().decode()
    assert (big == 7).all()
    b.expand.H, b.expand.W, b.project.H, b.project.W = 8 * stride, 8 * stride, 8, 8
    assert lib.load().hawq_linear_bottleneck_ok(C.byref(b)) == 1, (ho, wo)


# ------------------------------------------------------------------ e. global average pool at the int32 bound
POST8 = (5 << 27, 41, -128, 127)   # ratio 5 / 2^14: the 16-bit extremes land on -10 and 10


def _pool_expect(v, pre, post):
    """v [N][H W][C] int64 -> [N][C] in Python integers"""
    n, hw, c = v.shape
    out = np.zeros((n, c), np.int64)
    for i in range(n):
        for j in range(c):
            col = [int(t) for t in np.unique(v[i, :, j])]
            cnt = {t: int((v[i, :, j] == t).sum()) for t in col}
            s = sum(cnt[t] * (clamp(rne(t, pre[0], pre[1], 0), pre[2], pre[3]) if pre else t) for t in col)
            assert abs(100 * s + hw) <= CE.INT32_MAX
            r = CE.trunc_avg(s, hw)
            out[i, j] = clamp(rne(r, post[0], post[1], 0), post[2], post[3]) if post else r
    return out


@pytest.mark.parametrize("name", sorted(CE.POOL_BOUNDS))
@pytest.mark.parametrize("c", [16, 48])
@pytest.mark.parametrize("fill", ["lowest", "highest", "checkerboard"])
def test_global_pool_at_the_int32_bound(name, c, fill):
    from hawq_amd import _lib as L
    in_bits, pre, hw = CE.POOL_BOUNDS[name]
    h, w = CE.pool_shape(hw)
    assert h * w == hw and w <= 1024 and (name != "int16" or (h, w) == (5, 131))
    clamp_ = pre[2:] if pre else None
    assert CE.pool_global_takes(hw, in_bits, clamp_) and not CE.pool_global_takes(hw + 1, in_bits, clamp_)
    lo, hi = -(1 << (in_bits - 1)), (1 << (in_bits - 1)) - 1
    n = 2
    x = np.empty((n, hw, c), np.int16 if in_bits == 16 else np.int8)
    if fill == "checkerboard":
        x[:] = np.where((np.arange(hw)[None, :, None] + np.arange(c)[None, None, :] + np.arange(n)[:, None, None]) % 2 == 0, lo, hi)
    else:
        x[:] = lo if fill == "lowest" else hi
    xd = dev(x)
    for out_bits, post in ((16, None), (8, POST8)):
        want = _pool_expect(x.astype(np.int64), pre, post)
        out = out_buf(n * c, torch.int16 if out_bits == 16 else torch.int8, -3)
        a = L.IncepPoolArgs()
        a.in_, a.out = xd.data_ptr(), out.data_ptr()
        a.N, a.H, a.W, a.C, a.in_bits, a.in_pitch, a.out_bits, a.ldo = n, h, w, c, in_bits, c, out_bits, c
        if pre:
            a.pre, (a.m1, a.ek1, a.lo1, a.hi1) = 1, pre
        if post:
            a.post, (a.m2, a.ek2, a.lo2, a.hi2) = 1, post
        assert L.load().hawq_incep_pool_v_ok(C.byref(a), 3) == 1
        L.call("hawq_incep_pool_v", C.byref(a), 3, torch.cuda.current_stream().cuda_stream)
        got = out.cpu().numpy().astype(np.int64).reshape(n, c)
        assert np.array_equal(got, want), (name, fill, out_bits, got[0, :4], want[0, :4])
        if fill != "checkerboard" and not post:
            assert np.abs(want).max() > 100
        a.H, a.W = hw + 1, 1
        assert L.load().hawq_incep_pool_v_ok(C.byref(a), 3) == 0 and L.load().hawq_incep_pool_v(C.byref(a), 3, None) != 0


# ------------------------------------------------------------------ f. the weight-stationary kernel just under 2^23 pixels
@pytest.mark.parametrize("epi", ["requant", "residual"])
def test_weight_stationary_just_under_2_to_the_23_pixels(lib, orc, epi):
    """[2052][67][61]: M = 8 386 524 of the 8 388 607 the float-reciprocal division admits.  Image i is a copy of distinct image i % 3,
    repeated on the device; the oracle runs on the three.  Buffers of 0.5 to 1 GB; the case takes about 0.15 s on an MI355X,
    the host-side oracle included."""
    from hawq_amd.packing import pack_ctab
    from hawq_amd.quant_utils import requant_table, tables_are_fast
    n, h, w, c, distinct = 2052, 67, 61, 64, 3
    assert n * h * w == 8386524 < CE.PERSIST_PIXELS <= (n + 1) * h * w
    t0 = time.perf_counter()
    rng = np.random.default_rng(23)
    x, wt, b = K.make_conv(rng, distinct, h, w, c, c, 3, 8, 8)
    acc = orc.conv2d(x, wt, b, 1, 1)
    m, e = K.rand_tables(rng, c, 2e-5, 3e-4)
    assert tables_are_fast(m, e, int(np.abs(acc).max()).bit_length() + 1)
    idx = torch.arange(n, device="cuda") % distinct
    a, keep = K.conv_args(lib, x, wt, b, 1, 1, 8, 8)
    keep.update(ctab=dev(pack_ctab(b, m, e)), m=dev(m), e=dev(e))
    keep['xbig'] = dev(keep['x'].reshape(distinct, -1)[idx])
    a.in_, a.N = keep['xbig'].data_ptr(), n
    a.m, a.e, a.ctab, a.fast_tables = keep['m'].data_ptr(), keep['e'].data_ptr(), keep['ctab'].data_ptr(), 1
    out_q = out_buf(n * h * w * c, torch.uint8, 0x3C)
    a.out_q, a.out_bits = out_q.data_ptr(), 8
    if epi == "requant":
        a.epilogue, a.relu, a.q_lo, a.q_hi = lib.EPI_REQUANT, 1, -128, 127
        ref_q = K.odyadic(orc, np.maximum(acc, 0), m, e, (-128, 127))
    else:
        res = rng.integers(0, 60000, (distinct, c, h, w)).astype(np.int64)
        m1, e1 = requant_table(torch.tensor([0.37 * 0.7]), torch.ones(1), torch.tensor([0.7]))
        mq, eq = requant_table(torch.tensor([0.0039 * 0.7]), torch.ones(1), torch.tensor([0.7]))
        ref_res = np.maximum(K.odyadic(orc, acc, m, e) + K.odyadic(orc, res, m1, e1), 0)
        assert ref_res.max() < 65536
        ref_q = K.odyadic(orc, ref_res, mq, eq, (0, 127))
        keep['res'] = dev(torch.from_numpy(K.nhwc(res).astype(np.uint16).view(np.int16)).cuda().reshape(distinct, -1)[idx])
        flags = out_buf(1, torch.int32, 0)
        out_res = out_buf(n * h * w * c, torch.uint16, 0)
        a.epilogue, a.flags = lib.EPI_RESIDUAL, flags.data_ptr()
        a.res_in, a.res_in_bits, a.m_id_scalar, a.e_id_scalar = keep['res'].data_ptr(), 16, int(m1[0]), int(e1[0])
        a.res_out, a.res_out_bits = out_res.data_ptr(), 16
        a.q_lo, a.q_hi, a.mq, a.eq = 0, 127, int(mq[0]), int(eq[0])
    first = lib.load().hawq_conv2d_num_tiles() - lib.load().hawq_conv2d_num_band_tiles() + 1
    want_q = torch.from_numpy(K.nhwc(ref_q).astype(np.int8)).cuda().reshape(distinct, -1)
    for i, t in enumerate(CE.BAND_TILES):
        if not t.persist:
            continue
        a.tile, a.N = first + i, n
        out_q.fill_(0x3C)
        lib.call("hawq_conv2d", C.byref(a), K.stream())
        got = out_q.view(torch.int8).reshape(n, -1)
        for d in range(distinct):   # image i against distinct image i % 3, on the device
            assert bool((got[d::distinct] == want_q[d]).all()), (t.name, d)
        if epi == "residual":
            want_r = torch.from_numpy(K.nhwc(ref_res).astype(np.uint16).view(np.int16)).cuda().reshape(distinct, -1)
            for d in range(distinct):
                assert bool((out_res.view(torch.int16).reshape(n, -1)[d::distinct] == want_r[d]).all()), (t.name, d)
            assert flags.item() == 0
        a.N = n + 1   # 2053 images: 2^23 pixels and more
        assert lib.load().hawq_conv2d(C.byref(a), None) != 0
    print("weight-stationary kernel at M = %d, %s: %.2f s" % (n * h * w, epi, time.perf_counter() - t0))
