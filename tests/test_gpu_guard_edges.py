"""Directed guard-band cases: the smallest shapes at which the tail of a buffer can go wrong (one pixel, one pixel into a
second tile, rows narrower than the channel tile, the first and last image row of a 3x3 kernel), each compared with the
oracle by the case builder of the kernel family's own test file and run under two poisons, 0xA5 and 0x5A: a stray store
of one poison value, or an over-read that matches the expectation by chance, cannot hide under the other.  Every buffer
of every case comes from a tests/guard.py arena whose guards are checked when the case ends."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.test_gpu_band2 as B2
import tests.test_gpu_fused as F
import tests.test_gpu_gemm2 as G2
import tests.test_gpu_kernels as K
import tests.test_gpu_mbv2_kernels as MB
import tests.test_gpu_out_sub as OS
import tests.test_gpu_splitk as SK
import tests.test_gpu_stem_once as ST
from tests import guard
from tests.guard import dev, out_buf
from tests.test_gpu_kernels import lib, orc  # noqa: F401  (fixtures)

f32 = np.float32


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    prev = guard.set_current(ar)
    try:
        yield ar
    finally:
        guard.set_current(prev)
    ar.check()


pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("arena")]


def generic_tiles(lib):
    return list(range(0, lib.load().hawq_conv2d_num_tiles() - lib.load().hawq_conv2d_num_band_tiles() + 1))


def launch(lib, a, tile):
    """hawq_conv2d on tile id `tile`; every generic tile takes every case of this file (a refusal fails the caller's assert)."""
    a.tile = tile
    return lib.load().hawq_conv2d(C.byref(a), K.stream()) == 0


# ------------------------------------------------------------------ hawq_conv2d, 1x1, Cin = Cout = 64, every generic tile
M_SHAPES = [(1, 1, 1), (1, 7, 7), (1, 1, 257)]   # M = 1, 49 and 257: one pixel into a second 256-pixel tile


def _conv64(orc, nhw):
    n, h, w = nhw
    rng = np.random.default_rng(n * 1000 + h * 300 + w)
    x, wt, b = K.make_conv(rng, n, h, w, 64, 64, 1, 8, 8)
    return rng, x, wt, b, orc.conv2d(x, wt, b, 1, 0)


def _nchw(t, nhw, c=64):
    n, h, w = nhw
    return t.cpu().numpy().astype(np.int64).reshape(n, h, w, c).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("nhw", M_SHAPES)
def test_conv1x1_raw(lib, orc, nhw):
    rng, x, wt, b, acc = _conv64(orc, nhw)
    a, keep = K.conv_args(lib, x, wt, b, 1, 0, 8, 8)
    out = out_buf(acc.size, torch.int32, -7)
    a.epilogue, a.out_acc = lib.EPI_RAW, out.data_ptr()
    for tile in generic_tiles(lib):
        out.fill_(-7)
        assert launch(lib, a, tile), tile   # RAW is every generic tile's plainest form
        assert np.array_equal(_nchw(out, nhw), acc), tile


@pytest.mark.parametrize("nhw", M_SHAPES)
@pytest.mark.parametrize("out_bits", [8, 4])
@pytest.mark.parametrize("fast", [0, 1])
def test_conv1x1_requant(lib, orc, nhw, out_bits, fast):
    """REQUANT to 8 and 4 bits, NHWC on the exact and on the staged (fast-table) epilogue; with fast tables also planar."""
    from hawq_amd.packing import pack_ctab
    from hawq_amd.quant_utils import tables_are_fast
    n, h, w = nhw
    rng, x, wt, b, acc = _conv64(orc, nhw)
    m, e = K.rand_tables(rng, 64)
    assert tables_are_fast(m, e, int(np.abs(acc).max()).bit_length() + 1)
    lo, hi = (-128, 127) if out_bits == 8 else (0, 15)
    ref = K.odyadic(orc, np.maximum(acc, 0), m, e, (lo, hi))
    a, keep = K.conv_args(lib, x, wt, b, 1, 0, 8, 8)
    keep.update(m=dev(m), e=dev(e), ctab=dev(pack_ctab(b, m, e)))
    out = out_buf(acc.size * out_bits // 8, torch.uint8, 0)
    a.epilogue, a.relu, a.m, a.e = lib.EPI_REQUANT, 1, keep['m'].data_ptr(), keep['e'].data_ptr()
    a.out_q, a.out_bits, a.q_lo, a.q_hi = out.data_ptr(), out_bits, lo, hi
    if fast:
        a.fast_tables, a.ctab = 1, keep['ctab'].data_ptr()
    for tile in generic_tiles(lib):
        for planar in (0, 1) if fast else (0,):
            a.out_planar = planar
            out.fill_(0x3C)
            assert launch(lib, a, tile), (tile, planar)
            got = K.from_planar(out, (n, h, w, 64), out_bits) if planar else K.unpack_q(out, (n, h, w, 64), out_bits)
            assert np.array_equal(got, ref), (tile, planar)


@pytest.mark.parametrize("nhw", M_SHAPES)
@pytest.mark.parametrize("res_bits,fast", [(16, 0), (16, 1), (32, 0)])
def test_conv1x1_residual(lib, orc, nhw, res_bits, fast):
    """RESIDUAL with the uint16 and the int32 carrier, plus the next QuantAct's out_q."""
    from hawq_amd.packing import pack_ctab
    from hawq_amd.quant_utils import requant_table, tables_are_fast
    n, h, w = nhw
    rng, x, wt, b, acc = _conv64(orc, nhw)
    m2, e2 = K.rand_tables(rng, 64, 1e-3, 3e-2)
    res = rng.integers(0, 60000, (n, 64, h, w)).astype(np.int64)
    m1, e1 = requant_table(torch.tensor([0.37 * 0.7]), torch.ones(1), torch.tensor([0.7]))
    mq, eq = requant_table(torch.tensor([0.0039 * 0.7]), torch.ones(1), torch.tensor([0.7]))
    ref_res = np.maximum(K.odyadic(orc, acc, m2, e2) + K.odyadic(orc, res, m1, e1), 0)
    assert ref_res.max() < 65536
    ref_q = K.odyadic(orc, ref_res, mq, eq, (0, 127))
    assert tables_are_fast(m2, e2, int(np.abs(acc).max()).bit_length() + 1) and tables_are_fast(m1, e1, 17) and tables_are_fast(mq, eq, 17)
    a, keep = K.conv_args(lib, x, wt, b, 1, 0, 8, 8)
    keep.update(m=dev(m2), e=dev(e2), ctab=dev(pack_ctab(b, m2, e2)), res=dev(K.nhwc(res).astype(np.uint16 if res_bits == 16 else np.int32)))
    flags = out_buf(1, torch.int32, 0)
    out_res = out_buf(ref_res.size, torch.uint16 if res_bits == 16 else torch.int32, 0)
    out_q = out_buf(ref_res.size, torch.uint8, 0)
    a.epilogue, a.m, a.e, a.flags = lib.EPI_RESIDUAL, keep['m'].data_ptr(), keep['e'].data_ptr(), flags.data_ptr()
    a.res_in, a.res_in_bits, a.m_id_scalar, a.e_id_scalar = keep['res'].data_ptr(), res_bits, int(m1[0]), int(e1[0])
    a.res_out, a.res_out_bits = out_res.data_ptr(), res_bits
    a.out_q, a.out_bits, a.q_lo, a.q_hi, a.mq, a.eq = out_q.data_ptr(), 8, 0, 127, int(mq[0]), int(eq[0])
    if fast:
        a.fast_tables, a.ctab = 1, keep['ctab'].data_ptr()
    for tile in generic_tiles(lib):
        out_res.zero_(), out_q.fill_(0x3C)
        assert launch(lib, a, tile), tile
        assert np.array_equal(_nchw(out_res, nhw), ref_res), tile
        assert np.array_equal(K.unpack_q(out_q, (n, h, w, 64), 8), ref_q), tile
        assert flags.item() == 0


@pytest.mark.parametrize("nhw", M_SHAPES)
def test_conv1x1_dequant_leaves_the_gap_columns_alone(lib, orc, nhw):
    """DEQUANT with ldo > Cout and n_valid < Cout.  include/hawq_mi355.h: out_f32 is [M][ldo] fp32 and "only channels < n_valid
    are written": columns n_valid .. ldo - 1 of every row keep what they held."""
    LDO, NV = 80, 40
    rng, x, wt, b, acc = _conv64(orc, nhw)
    M = acc.size // 64
    fs = rng.uniform(1e-5, 1e-3, 64).astype(f32)
    ref = (K.nhwc(acc).reshape(M, 64).astype(f32) * fs.reshape(1, -1)).astype(f32)[:, :NV]
    a, keep = K.conv_args(lib, x, wt, b, 1, 0, 8, 8)
    keep['fs'] = dev(fs)
    out = out_buf((M, LDO), torch.float32, -7.0)
    a.epilogue, a.out_f32, a.fscale, a.ldo, a.n_valid = lib.EPI_DEQUANT, out.data_ptr(), keep['fs'].data_ptr(), LDO, NV
    for tile in generic_tiles(lib):
        out.fill_(-7.0)
        assert launch(lib, a, tile), tile
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :NV], ref), tile
        assert (got[:, NV:] == f32(-7.0)).all(), tile


# ------------------------------------------------------------------ narrow tensors: the last pixel row is where an excess store survives
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("mode", ["closing_clamp16", "closing_identity", "requant"])
@pytest.mark.parametrize("widths", [(24, 32, 16, 16), (16, 16, 24, 32), (96, 96, 40, 48)])
@pytest.mark.parametrize("nhw", [(1, 1, 1), (1, 3, 3)])
def test_narrow_tensors_on_tiny_maps(lib, orc, nhw, widths, mode, fast):
    MB.test_conv2d_on_narrow_tensors(lib, orc, widths, mode, fast, nhw=nhw)


# ------------------------------------------------------------------ 3x3 kernels: first and last image rows
BAND_SHAPES = [(1, 3, 5, 64, 64), (1, 7, 7, 128, 128), (2, 7, 7, 64, 64)]


@pytest.mark.parametrize("shape", BAND_SHAPES)
@pytest.mark.parametrize("bits", [8, 4])
def test_band_and_weight_stationary_requant(lib, orc, shape, bits):
    """band tiles and the weight-stationary kernel: REQUANT, NHWC and planar in and out; hawq4 operands where Cin % 128 == 0
    (any other W4A4 case is refused by every band tile, which the builder asserts)."""
    K.test_conv3x3_band_kernels(lib, orc, shape, bits)


@pytest.mark.parametrize("shape", BAND_SHAPES)
@pytest.mark.parametrize("bits,mode", [(8, 1), (8, 5), (4, 1)])
def test_band_and_weight_stationary_residual(lib, orc, shape, bits, mode):
    K.test_conv3x3_band_residual(lib, orc, shape, bits, mode)


def _band2_takes(lib, shape, bits=8):
    n, h, w, cin, cout = shape
    return [t for t, (bm, band_px) in zip(B2._ids(lib), B2.GEOM2) if B2._applies(bm, band_px, w, cin, bits)]


@pytest.mark.parametrize("shape", [(1, 3, 5, 64, 64), (2, 7, 7, 64, 64)])
def test_band2_refuses_the_64_channel_cases(lib, orc, shape):
    """band_v2 wants a 128-byte pixel row: it refuses Cin = 64, and the next smallest cases it takes follow below."""
    n, h, w, cin, cout = shape
    assert not _band2_takes(lib, shape)
    rng = np.random.default_rng(1)
    x, wt, b = K.make_conv(rng, n, h, w, cin, cout, 3, 8, 8)
    for tile in B2._ids(lib):
        a, keep = B2._args(lib, x, wt, b, tile)
        out = out_buf(n * h * w * cout, torch.int32, -7)
        a.epilogue, a.out_acc = lib.EPI_RAW, out.data_ptr()
        assert lib.load().hawq_conv2d(C.byref(a), None) != 0, tile
        assert (out == -7).all()


BAND2_SHAPES = [(1, 3, 5, 128, 64), (1, 7, 7, 128, 128), (2, 7, 7, 128, 64)]


@pytest.mark.parametrize("shape", BAND2_SHAPES)
@pytest.mark.parametrize("mode", [1, 5])
def test_band2_requant_and_residual(lib, orc, shape, mode):
    B2.test_band2_requant(lib, orc, shape, mode)
    B2.test_band2_residual(lib, orc, shape, mode)


@pytest.mark.parametrize("shape", [(1, 3, 5, 256, 64), (1, 7, 7, 256, 128)])
def test_band2_hawq4(lib, orc, shape):
    """hawq4 operands need Cin % 128 == 0 and two 64-byte slices: Cin = 256 is the smallest the kernels take."""
    assert _band2_takes(lib, shape, 4)
    B2.test_band2_hawq4_operands_and_outputs(lib, orc, shape, 1)
    B2.test_band2_raw_accumulators(lib, orc, shape, 4)


# ------------------------------------------------------------------ gemm2 (streaming 1x1) tiles
@pytest.mark.parametrize("shape", [(1, 3, 3, 512, 64, 1), (1, 1, 1, 256, 128, 1)])
@pytest.mark.parametrize("mode", [1, 5])
def test_gemm2_tiny_maps(lib, orc, shape, mode):
    G2.test_gemm2_requant(lib, orc, shape, mode)
    G2.test_gemm2_residual(lib, orc, shape[:5], mode)
    if mode == 1:
        G2.test_gemm2_raw_accumulators(lib, orc, shape, 8)


@pytest.mark.parametrize("mode", [1, 5])
def test_gemm2_dual_branch_smallest(lib, orc, mode):
    G2.test_gemm2_residual_with_identity_conv(lib, orc, min(G2.DUAL_SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[4]), mode)


# ------------------------------------------------------------------ out_sub
@pytest.mark.parametrize("tie", [False, True])
def test_out_sub_smallest_odd_map(lib, orc, tie):
    shape = OS.SHAPES[0]
    assert shape[1] % 2 == 1 and shape[2] % 2 == 1
    OS.test_solo_kernel_equals_the_dense_launch_gathered(lib, orc, OS.CHANNELS[0], shape, tie)
    if not tie:
        OS.test_solo_kernel_equals_the_oracle(lib, orc, OS.CHANNELS[0])
        for res_bits, fast in ((16, True), (32, False)):
            OS.test_generic_path_equals_the_dense_launch_gathered(lib, orc, OS.CHANNELS[0], shape, res_bits, fast)


# ------------------------------------------------------------------ split-K: workspace and counters under guard
@pytest.mark.parametrize("hw,cin,cout,k", [((1, 1), 512, 512, 1), ((7, 7), 512, 512, 3), ((7, 7), 512, 2048, 1)])
def test_splitk_single_pixel_and_ragged_tile(lib, orc, hw, cin, cout, k):
    """M = 1 and M = 49 at the largest slice count the entry point accepts: RAW against the oracle, REQUANT byte for byte against
    hawq_conv2d; the workspace is exactly as large as hawq_conv2d_splitk_workspace says."""
    from hawq_amd.quant_utils import tables_are_fast
    h, w = hw
    rng = np.random.default_rng(h * 10 + k + cout)
    x, wt, b = K.make_conv(rng, 1, h, w, cin, cout, k, 8, 8)
    acc = orc.conv2d(x, wt, b, 1, k // 2)
    ref = K.nhwc(acc)
    a, keep = K.conv_args(lib, x, wt, b, 1, k // 2, 8, 8)
    out = out_buf(ref.size, torch.int32, -1)
    a.epilogue, a.out_acc = lib.EPI_RAW, out.data_ptr()
    slices = SK.accepted(lib, a)
    assert slices, "split-K refuses the case"
    for s in SK.CANDIDATES:
        if s not in slices:
            assert lib.load().hawq_conv2d_splitk(C.byref(a), s, None, None, None) != 0, s
    s = max(slices)
    ws = SK.workspace(lib, a, s)
    SK.splitk(lib, a, s, ws)
    assert np.array_equal(out.cpu().numpy().reshape(ref.shape), ref), s
    assert int(ws[1].abs().sum()) == 0
    m, e = K.rand_tables(rng, cout, 2e-5, 3e-4)
    assert tables_are_fast(m, e, int(np.abs(acc).max()).bit_length() + 1)
    SK._tables(lib, keep, a, b, m, e, 1)
    a.epilogue, a.out_acc, a.relu, a.out_bits, a.q_lo, a.q_hi = lib.EPI_REQUANT, None, 1, 8, -128, 127
    t = SK._outputs(a, h * w, cout)
    assert max(SK._compare_with_conv2d(lib, a, t)) == s


# ------------------------------------------------------------------ fused expand + reduce: pair, wave-private, dual-branch
ER_SHAPES = [(1, 3, 5, 64, 64), (1, 1, 1, 64, 256)]


@pytest.mark.parametrize("shape", ER_SHAPES)
@pytest.mark.parametrize("tie", [False, True])
def test_expand_reduce_pair(lib, orc, shape, tie):
    F.test_expand_reduce_matches_oracle(lib, orc, shape, tie)   # every variant hawq_conv_expand_reduce_variants reports


@pytest.mark.parametrize("shape", ER_SHAPES)
@pytest.mark.parametrize("tie", [False, True])
def test_expand_alone_wave_private(lib, orc, shape, tie):
    F.test_expand_alone_wave_private(lib, orc, shape, tie)


@pytest.mark.parametrize("shape", ER_SHAPES)
@pytest.mark.parametrize("tie", [False, True])
def test_expand_reduce_dual_branch(lib, orc, shape, tie):
    F.test_expand_reduce_dual_branch(lib, orc, shape, tie)


# ------------------------------------------------------------------ MobileNetV2: one-launch units, depthwise convs, stem
def _unit_tiles(unit):
    ipitch, opitch = unit[1], unit[4]
    return [t for t in range(5) if not (t == 1 and max(ipitch, opitch) > 64) and not (t > 1 and max(ipitch, opitch) > 96)]


LB_UNITS = [u for u in MB.UNITS if u[7] in ((1, 5, 8), (1, 7, 9))] + [MB.UNITS[1][:7] + ((1, 3, 3),) + MB.UNITS[1][8:]]


@pytest.mark.parametrize("unit,tile", [(u, t) for u in LB_UNITS for t in _unit_tiles(u)])
def test_linear_bottleneck_small_maps(lib, orc, unit, tile):
    MB.test_linear_bottleneck_against_the_oracle(lib, orc, unit, tile)


def test_linear_bottleneck_cases_are_the_intended_ones():
    assert sorted(u[7] for u in LB_UNITS) == [(1, 3, 3), (1, 5, 8), (1, 7, 9)] and LB_UNITS[-1][5] == 2


@pytest.mark.parametrize("shape", [(2, 3, 3, 4, 2), (1, 5, 6, 8, 2)])
def test_depthwise_stride2_tiny(lib, orc, shape):
    K.test_depthwise3x3_matches_the_grouped_kernel_and_numpy(lib, shape)
    for relu in (0, 1):
        K.test_depthwise3x3_requant_matches_accumulators_plus_host_dyadic(lib, orc, shape + (relu,))


@pytest.mark.parametrize("shape", [(2, 3, 3, 16, 4, 2), (1, 5, 6, 16, 8, 2)])
@pytest.mark.parametrize("tie", [False, True])
def test_depthwise_fast_stride2_tiny(lib, orc, shape, tie):
    MB.test_depthwise3x3_requant_fast_against_the_oracle(lib, orc, shape, tie)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("hw", [(9, 7), (33, 46)])
def test_stem3x3s2(lib, orc, hw, u8):
    MB.test_stem3x3s2_against_the_oracle(lib, orc, hw, u8)


# ------------------------------------------------------------------ ResNet stem, pools, classifier
@pytest.mark.parametrize("shape", [ST.SMALL[0], (1, 35, 51)])
def test_fused_stems_both_input_types(lib, orc, shape):
    """hawq_stem_fused and hawq_stem_fused_u8, both outputs and either alone: the smallest map, and a width that is no
    multiple of the stem tile."""
    ST.test_stem_tile_seams_and_small_maps(lib, orc, shape)


def test_maxpool_and_requant_residual(lib, orc):
    K.test_quantize_input_and_stem(lib, orc)


@pytest.mark.parametrize("res_bits", [16, 32])
@pytest.mark.parametrize("c", [512, 320])
def test_avgpool(lib, orc, res_bits, c):
    K.test_avgpool_requant(lib, orc, res_bits, c)


@pytest.mark.parametrize("n,k,nout", [(1, 512, 10), (33, 128, 33)])
def test_fc_dequant(lib, orc, n, k, nout):
    K.test_fc_dequant_kernel_equals_the_conv_kernels_dequant_epilogue(lib, orc, n, k, nout)


# ------------------------------------------------------------------ fp32-convention adapters
@pytest.mark.parametrize("c,cpad", [(3, 8), (64, 64)])
@pytest.mark.parametrize("bits", [8, 4])
def test_adapters_on_a_3x5_map(lib, c, cpad, bits):
    """hawq_f32_nchw_to_q_nhwc (extra channels zero) and hawq_acc_nhwc_to_f32_nchw on a 3 x 5 map.  The quantiser packs eight
    channels per store, so a pad to 4 channels is refused and 8 is the smallest pad of a 3-channel image."""
    from hawq_amd.packing import unpack_hawq4
    n, h, w = 2, 3, 5
    rng = np.random.default_rng(c + bits)
    lo, hi = (-128, 127) if bits == 8 else (0, 15)
    scale = f32(0.037)
    q = rng.integers(lo, hi + 1, (n, c, h, w))
    x = (q.astype(f32) * scale + rng.uniform(-0.4, 0.4, q.shape).astype(f32) * scale).astype(f32)
    ref = np.rint(x / scale).astype(np.int64)
    xd = dev(x)
    out = out_buf(n * h * w * cpad * bits // 8, torch.uint8, 0x3C)
    if c == 3:
        assert lib.load().hawq_f32_nchw_to_q_nhwc(xd.data_ptr(), out.data_ptr(), n, c, h, w, 4, bits, float(scale), None) != 0
        assert (out == 0x3C).all()
    lib.call("hawq_f32_nchw_to_q_nhwc", xd.data_ptr(), out.data_ptr(), n, c, h, w, cpad, bits, float(scale), K.stream())
    raw = out.cpu().numpy()
    got = raw.view(np.int8).astype(np.int64).reshape(n, h, w, cpad) if bits == 8 else unpack_hawq4(raw.reshape(n, h, w, cpad // 2)).astype(np.int64)
    assert np.array_equal(got[..., :c].transpose(0, 3, 1, 2), ref)
    assert not got[..., c:].any()
    acc = rng.integers(-2 ** 30, 2 ** 30, (n, h, w, cpad)).astype(np.int32)
    fs = rng.uniform(1e-5, 1e-3, cpad).astype(f32)
    ad, fd = dev(acc), dev(fs)
    y = out_buf((n, c, h, w), torch.float32, -7.0)
    lib.call("hawq_acc_nhwc_to_f32_nchw", ad.data_ptr(), y.data_ptr(), n, c, h, w, cpad, fd.data_ptr(), K.stream())
    want = (acc[..., :c].astype(f32) * fs[:c]).astype(f32).transpose(0, 3, 1, 2)
    assert np.array_equal(y.cpu().numpy(), want)
