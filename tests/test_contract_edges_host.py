"""The restatements of tests/contract_edges.py against the built library's host-only queries: every capacity rule accepts exactly
where its restatement does, the accepted runs are the pinned ones, and band_persist's float-reciprocal division is exact over its
admitted range.  No device."""
import ctypes as C

import numpy as np
import pytest

from hawq_amd import _lib
from tests import contract_edges as CE
from tests.conv_choice_cases import PACKED, PTR, RAW, REQUANT, RES16, conv, with_fast

H_FIXED = 9


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _accepts(lib, a):
    return lib.hawq_conv2d_choice(C.byref(a), C.byref(_lib.ConvChoice())) == 0


def _band_ids(lib):
    """(ids of the band_v1 and weight-stationary tiles, ids of the band_v2 tiles)"""
    n, nsp, nb2, ng2 = lib.hawq_conv2d_num_tiles(), lib.hawq_conv2d_num_band_tiles(), lib.hawq_conv2d_num_band2_tiles(), lib.hawq_conv2d_num_gemm2_tiles()
    first = n - nsp + 1
    return list(range(first, n - ng2 - nb2 + 1)), list(range(n - ng2 - nb2 + 1, n - ng2 + 1))


def _layer(w, cin, cout, epi, **kw):
    a = conv(2, H_FIXED, cin, cout, 3, 1, **with_fast(dict(epi, **kw), 1))
    a.W = w
    return a


# ---------------------------------------------------------------------------------------------- band tile widths
def test_the_tile_tables_have_the_library_s_length(lib):
    v1, v2 = _band_ids(lib)
    assert len(v1) == len(CE.BAND_TILES) and len(v2) == len(CE.BAND2_TILES)
    assert set(CE.BAND_RUNS) == {t.name for t in CE.BAND_TILES}


@pytest.mark.parametrize("index", range(len(CE.BAND_TILES)), ids=[t.name for t in CE.BAND_TILES])
@pytest.mark.parametrize("epi", ["requant", "res16"])
def test_band_v1_and_weight_stationary_widths(lib, index, epi):
    t = CE.BAND_TILES[index]
    tile = _band_ids(lib)[0][index]
    c = t.bn   # Cin = Cout = the tile's channel tile: 64 for B0, B5 and the weight-stationary kernel, else 128
    got = CE.runs(lambda w: _accepts(lib, _layer(w, c, c, REQUANT if epi == "requant" else RES16, tile=tile)))
    assert got == CE.band_runs(t), (t.name, "the library and the restatement disagree")
    assert got == CE.BAND_RUNS[t.name], (t.name, "the tile's LDS geometry moved")
    for w in CE.WIDTHS:
        assert (index in CE.band_takers(w, c, c)) == any(a <= w <= b for a, b in got)


def test_band_v1_hawq4_and_slice_rules(lib):
    """hawq4 operands need Cin % 128 == 0; B0 and the weight-stationary kernel take one 64-byte slice; Cout is a multiple of the tile's"""
    ids = _band_ids(lib)[0]
    for cin, cout, bits in ((64, 64, 8), (128, 128, 8), (256, 128, 8), (128, 64, 8), (64, 64, 4), (128, 128, 4), (256, 128, 4), (128, 64, 4), (192, 128, 4)):
        for w in (3, 29, 34, 61, 70):
            got = [i for i, tile in enumerate(ids) if _accepts(lib, _layer(w, cin, cout, REQUANT, tile=tile, in_bits=bits, w_bits=bits))]
            assert got == CE.band_takers(w, cin, cout, bits), (cin, cout, bits, w)


def test_every_upper_run_end_is_within_eight_pixels_of_a_full_band():
    for t in CE.BAND_TILES:
        for a, b in CE.band_runs(t):
            assert 0 <= CE.band_slack(t, b) <= 8, (t.name, b)
            assert CE.band_slack(t, b + 1) < 0 and CE.band_slack(t, a - 1) < 0
    assert CE.BAND_WIDTHS == [3, 6, 27, 29, 32, 34, 61, 64, 70]
    for n, v in CE.BAND_REFUSED.items():
        assert set(CE.first_refused(CE.BAND_RUNS[n])) | {1, 2} == set(v), n


@pytest.mark.parametrize("index", range(len(CE.BAND2_TILES)), ids=[t.name for t in CE.BAND2_TILES])
@pytest.mark.parametrize("epi", ["requant", "res16", "raw"])
def test_band_v2_widths(lib, index, epi):
    t = CE.BAND2_TILES[index]
    tile = _band_ids(lib)[1][index]
    fields = {"requant": REQUANT, "res16": RES16, "raw": RAW}[epi]
    got = CE.runs(lambda w: _accepts(lib, _layer(w, 128, 128, fields, tile=tile, in_planar=1, **PACKED)))
    assert got == CE.runs(lambda w: CE.band2_fits(t, w)) == CE.BAND2_RUNS
    assert CE.band2_used(t.bm, 57) == t.band_px - 4 - 1   # one pixel short of the stage


# ---------------------------------------------------------------------------------------------- strided twins
def _walk_worst(lib, a, index):
    ext = (C.c_int32 * 5)()
    assert lib.hawq_conv2d_band2_sub_extent(C.byref(a), index, 0, ext) == 0
    worst = 0
    for tile in range(ext[3]):
        assert lib.hawq_conv2d_band2_sub_extent(C.byref(a), index, tile, ext) == 0
        worst = max(worst, ext[1])
    return worst, ext[2], ext[4]


@pytest.mark.parametrize("index", range(len(CE.BAND2_TILES)), ids=[t.name for t in CE.BAND2_TILES])
def test_strided_twins_widest_source_width(lib, index):
    t = CE.BAND2_TILES[index]
    tile = _band_ids(lib)[1][index]
    accepted = []
    for w in CE.SUB_SEARCH:
        a = conv(CE.SUB_N, CE.SUB_H, 128, 128, 3, 1, **with_fast(dict(REQUANT, out_sub=2, in_planar=1, tile=tile, **PACKED), 1))
        a.W = w
        worst, band_px, bm = _walk_worst(lib, a, index)
        assert (bm, band_px) == (t.sub_bm, t.sub_band_px)
        assert worst == CE.band2_sub_worst(CE.SUB_N, CE.SUB_H, w, bm), w
        assert _accepts(lib, a) == (worst <= band_px - 4) == CE.band2_sub_fits(t, CE.SUB_N, CE.SUB_H, w), w
        if worst <= band_px - 4:
            accepted.append(w)
    widest = max(accepted)
    assert widest == CE.band2_sub_widest(t) and widest + 1 not in accepted
    assert CE.band2_sub_worst(CE.SUB_N, CE.SUB_H, widest + 1, t.sub_bm) > t.sub_band_px - 4   # one column more and a tile spans a further row
    assert widest == CE.SUB_WIDEST[t.name]


# ---------------------------------------------------------------------------------------------- the other checks
def test_wide_bottleneck_units_end_at_8_by_8(lib):
    for cin, ip, hid, cout, op, stride, identity, nhw, small in CE.LB_WIDE_UNITS:
        assert CE.lb_wide_takes(nhw[1], nhw[2], stride)
        assert lib.hawq_linear_bottleneck_ok(C.byref(CE.bottleneck_args(ip, op, stride, nhw))) == 1, lib.hawq_last_error().decode()
    for cin, cout, stride, (h, w) in CE.LB_WIDE_REFUSED:
        assert not CE.lb_wide_takes(h, w, stride)
        assert lib.hawq_linear_bottleneck_ok(C.byref(CE.bottleneck_args(cin, cout, stride, (2, h, w)))) == 0
    # the same maps on a unit of at most 96 channels are taken: the 8 x 8 rule is the wide family's alone
    assert lib.hawq_linear_bottleneck_ok(C.byref(CE.bottleneck_args(96, 96, 1, (2, 9, 8)))) == 1


def _pool(h, w, in_bits, pre):
    a = _lib.IncepPoolArgs()
    a.in_, a.out = PTR, PTR
    a.N, a.H, a.W, a.C, a.in_bits, a.in_pitch, a.out_bits, a.ldo = 2, h, w, 16, in_bits, 16, 16, 16
    if pre:
        a.pre, (a.m1, a.ek1, a.lo1, a.hi1) = 1, pre
    return a


@pytest.mark.parametrize("name", sorted(CE.POOL_BOUNDS))
def test_global_pool_int32_bound(lib, name):
    in_bits, pre, hw = CE.POOL_BOUNDS[name]
    clamp = pre[2:] if pre else None
    assert CE.pool_global_max_hw(in_bits, clamp) == hw
    assert CE.pool_global_takes(hw, in_bits, clamp) and not CE.pool_global_takes(hw + 1, in_bits, clamp)
    bound = CE.pool_bound(in_bits, clamp)
    assert 100 * bound * hw + hw <= CE.INT32_MAX < 100 * bound * (hw + 1) + hw + 1   # the last H W at which 100 s + H W fits
    for shape, want in (((hw, 1), 1), ((hw + 1, 1), 0), (CE.pool_shape(hw), 1), ((1, hw), 1), ((1, hw + 1), 0)):
        assert lib.hawq_incep_pool_v_ok(C.byref(_pool(*shape, in_bits, pre)), _lib.INCEP_POOL_OPS["hawq_incep_global_avgpool"]) == want, shape
    h, w = CE.pool_shape(hw)
    assert h * w == hw and w <= 1024
    if name == "int16":
        assert (h, w) == (5, 131)


def test_weight_stationary_pixel_count(lib):
    """N H W < 2^23.  2^23 - 1 = 47 * 178481, so the last accepted count is a [178481][1][47] launch; 2^23 itself is [131072][1][64]."""
    ids = _band_ids(lib)[0]
    for tile in ids[-2:]:
        for n, h, w, want in ((178481, 1, 47, True), (131072, 1, 64, False), (131071, 1, 64, True), (2052, 67, 61, True), (2053, 67, 61, False)):
            for epi in (REQUANT, RES16):
                a = conv(n, h, 64, 64, 3, 1, **with_fast(dict(epi, tile=tile), 1))
                a.W = w
                assert (n * h * w < CE.PERSIST_PIXELS) == want
                assert _accepts(lib, a) == want, (tile, n, h, w)
    assert 178481 * 47 == CE.PERSIST_PIXELS - 1 and 2052 * 67 * 61 == 8386524
    # band_v1's B0 has no such bound: it divides in integers
    a = conv(2053, 67, 64, 64, 3, 1, **with_fast(dict(REQUANT, tile=ids[0]), 1))
    a.W = 61
    assert _accepts(lib, a)


# ---------------------------------------------------------------------------------------------- fdiv
@pytest.mark.parametrize("d", sorted(set(range(3, 71)) | {CE.band_seam_height(w) for w in CE.BAND_WIDTHS} | {67, H_FIXED}))
def test_fdiv_in_float32_is_floor_division_below_2_to_the_23(d):
    """every multiple of d below 2^23 and its two neighbours: the places where a truncated float quotient can be one off"""
    k = np.arange(0, CE.PERSIST_PIXELS // d + 2, dtype=np.int64) * d
    m = np.concatenate([k - 1, k, k + 1, [CE.PERSIST_PIXELS - 1]])
    m = m[(m >= 0) & (m < CE.PERSIST_PIXELS)]
    assert m.max() == CE.PERSIST_PIXELS - 1
    assert np.array_equal(CE.fdiv_f32(m, d), m // d)
    # the estimate alone is not the quotient: the corrections are needed, and one step of each suffices
    r = np.float32(1.0) / np.float32(d)
    est = (m.astype(np.float32) * r).astype(np.int64)
    assert np.abs(est - m // d).max() <= 1


def test_fdiv_restatement_notices_a_missing_correction():
    m = np.arange(0, 1 << 16, dtype=np.int64)
    wrong = 0
    for d in (3, 5, 7, 61):
        r = np.float32(1.0) / np.float32(d)
        wrong += int(((m.astype(np.float32) * r).astype(np.int64) != m // d).sum())
    assert wrong > 0


# ---------------------------------------------------------------------------------------------- the case lists
def test_seam_heights_reach_the_seams():
    for w in CE.BAND_WIDTHS:
        h = CE.band_seam_height(w)
        bms = {t.bm for t in CE.BAND_TILES if CE.band_fits(t.bm, t.band_px, w)}
        assert bms and all(CE.tile_facts(2, h, w, bm) for bm in bms), w
    for w in (1, 2, 57):
        assert all(CE.tile_facts(2, CE.seam_height(w), w, bm) for bm in (128, 256)), w


def test_stem_shapes_have_the_chunks_they_claim():
    assert CE.STEM_CW == 159
    for (n, h, w), want in CE.STEM_SHAPES.items():
        assert CE.stem_chunks(w)[1:] == want
    assert sorted(v[0] for v in CE.STEM_SHAPES.values()) == [1, 2, 2, 2, 3]
