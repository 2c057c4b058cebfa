"""GPU tests of the cross-workgroup split-K conv kernel (hawq_conv2d_splitk, conv_splitk.hip).

RAW accumulators are compared with the CPU oracle; the REQUANT / RESIDUAL outputs (out_q, res_out, *flags) are compared byte for
byte with hawq_conv2d on the same arguments, whose epilogues the split-K kernel shares."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard import guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_kernels import conv_args, dev, make_conv, nhwc, pack_act, rand_tables, stream, to_planar

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]

CANDIDATES = (2, 4, 8, 16, 32)

# (h, w, cin, cout, k, stride) of stage 2-4 layers; h, w are the INPUT extents
LAYERS = {
    "resnet50.stage2.conv2": (28, 28, 128, 128, 3, 1),
    "resnet50.stage3.conv1": (14, 14, 1024, 256, 1, 1),
    "resnet50.stage3.conv2": (14, 14, 256, 256, 3, 1),
    "resnet50.stage4.conv2": (7, 7, 512, 512, 3, 1),          # M = 49 at batch 1
    "resnet50.stage4.conv3": (7, 7, 512, 2048, 1, 1),
    "resnet50.stage4.unit1.conv1s2": (14, 14, 1024, 512, 1, 2),
    "resnet50b.stage4.unit1.conv2s2": (14, 14, 512, 512, 3, 2),
    "resnet18.stage3.unit1.conv1s2": (28, 28, 128, 256, 3, 2),
    "resnet18.stage4.conv2": (7, 7, 512, 512, 3, 1),
}


@pytest.fixture(scope="module")
def lib():
    from hawq_amd import _lib
    _lib.load()
    _lib.check(_lib.load().hawq_device_ok())
    return _lib


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def workspace(lib, a, s):
    slab, cnt = C.c_int64(), C.c_int64()
    lib.call("hawq_conv2d_splitk_workspace", C.byref(a), s, C.byref(slab), C.byref(cnt))
    return (out_buf(slab.value, torch.uint8, 0x5a),   # garbage: every slab byte is written before it is read
            out_buf(cnt.value // 4, torch.int32, 0))


def splitk(lib, a, s, ws):
    lib.call("hawq_conv2d_splitk", C.byref(a), s, ws[0].data_ptr(), ws[1].data_ptr(), stream())


def accepted(lib, a):
    return [s for s in CANDIDATES if lib.load().hawq_conv2d_splitk_ok(C.byref(a), s)]


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_raw_accumulators_equal_the_oracle_for_every_slice_count(lib, orc, layer, n):
    h, w, cin, cout, k, stride = LAYERS[layer]
    pad = k // 2
    rng = np.random.default_rng(hash(layer) % 1000 + n)
    x, wt, b = make_conv(rng, n, h, w, cin, cout, k, 8, 8)
    ref = nhwc(orc.conv2d(x, wt, b, stride, pad))
    a, keep = conv_args(lib, x, wt, b, stride, pad, 8, 8)
    out = out_buf(ref.size, torch.int32, 0)
    a.epilogue, a.out_acc = lib.EPI_RAW, out.data_ptr()
    slices = accepted(lib, a)
    assert slices and slices[0] == 2
    for s in slices:
        out.fill_(-1)
        ws = workspace(lib, a, s)
        splitk(lib, a, s, ws)
        assert np.array_equal(out.cpu().numpy().reshape(ref.shape), ref), s
        assert int(ws[1].abs().sum()) == 0, s   # every arrival counter back at zero


def _tables(lib, keep, a, b, m, e, mode):
    from hawq_amd.packing import pack_ctab
    keep.update(m=dev(m), e=dev(e), ctab=dev(pack_ctab(b, m, e)))
    a.m, a.e, a.fast_tables = keep['m'].data_ptr(), keep['e'].data_ptr(), mode
    if mode:
        a.ctab = keep['ctab'].data_ptr()


def _outputs(a, M, cout, res_bits=16):
    t = dict(q=out_buf(M * cout, torch.uint8, 0),
             res=out_buf(M * cout, torch.uint16 if res_bits == 16 else torch.int32, 0),
             flags=out_buf(1, torch.int32, 0))
    a.out_q, a.flags = t['q'].data_ptr(), t['flags'].data_ptr()
    if a.epilogue == 2:
        a.res_out, a.res_out_bits = t['res'].data_ptr(), res_bits
    return t


def _snapshot(t):
    return {k: v.cpu().numpy().copy() for k, v in t.items()}


def _compare_with_conv2d(lib, a, t, planar_in=None, expect_flag=None):
    """hawq_conv2d on `a` (NHWC input), then hawq_conv2d_splitk on `a` (planar input if given) for every accepted slice count:
    identical bytes in every output."""
    lib.call("hawq_conv2d", C.byref(a), stream())
    ref = _snapshot(t)
    if expect_flag is not None:
        assert int(ref['flags'][0]) & 1 == expect_flag
    if planar_in is not None:
        a.in_, a.in_planar = planar_in.data_ptr(), 1
    slices = accepted(lib, a)
    assert slices
    for s in slices:
        for v in t.values():
            v.fill_(0x33 if v.dtype == torch.uint8 else 0)
        ws = workspace(lib, a, s)
        splitk(lib, a, s, ws)
        got = _snapshot(t)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (s, k)
        assert int(ws[1].abs().sum()) == 0
    return slices


TABLES = {"fast": 1, "tie": 5, "general": 0}


@pytest.mark.parametrize("layout", ["nhwc", "planar"])
@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("layer,n", [("resnet50.stage4.conv2", 1), ("resnet50.stage3.conv1", 3), ("resnet50b.stage4.unit1.conv2s2", 1)])
def test_requant_epilogue_is_byte_identical_to_hawq_conv2d(lib, layer, n, relu, tables, layout):
    if layout == "planar" and not TABLES[tables]:
        return _requant_general_refuses_planar(lib)
    h, w, cin, cout, k, stride = LAYERS[layer]
    rng = np.random.default_rng(5 + relu + n)
    x, wt, b = make_conv(rng, n, h, w, cin, cout, k, 8, 8)
    a, keep = conv_args(lib, x, wt, b, stride, k // 2, 8, 8)
    m, e = rand_tables(rng, cout, 2e-5, 3e-4)
    _tables(lib, keep, a, b, m, e, TABLES[tables])
    a.epilogue, a.relu, a.out_bits, a.q_lo, a.q_hi = lib.EPI_REQUANT, relu, 8, -128, 127
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    t = _outputs(a, n * ho * wo, cout)
    if layout == "planar":
        a.out_planar = 1
        keep['xp'] = dev(to_planar(pack_act(x, 8)))
    _compare_with_conv2d(lib, a, t, keep.get('xp'))


def _requant_general_refuses_planar(lib):
    # planar input is taken with the fast-contract epilogues only (the engine writes planes only for those launches)
    a = lib.ConvArgs()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad, a.in_bits, a.w_bits = 1, 7, 7, 512, 512, 3, 3, 1, 1, 8, 8
    a.epilogue, a.out_q, a.out_bits, a.in_planar, a.fast_tables = 1, 1, 8, 1, 0
    assert lib.load().hawq_conv2d_splitk_ok(C.byref(a), 2) == 0
    a.in_planar = 0
    assert lib.load().hawq_conv2d_splitk_ok(C.byref(a), 2) == 1


def _residual_case(lib, rng, layer, n, tables, dual, res_bits=16, big_res=False):
    from hawq_amd.packing import pack_conv_weight
    from hawq_amd.quant_utils import requant_table
    h, w, cin, cout, k, stride = LAYERS[layer]
    x, wt, b = make_conv(rng, n, h, w, cin, cout, k, 8, 8)
    a, keep = conv_args(lib, x, wt, b, stride, k // 2, 8, 8)
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    m2, e2 = rand_tables(rng, cout, 2e-5, 3e-4)
    _tables(lib, keep, a, b, m2, e2, TABLES[tables])
    a.epilogue = lib.EPI_RESIDUAL
    if dual:   # the identity 1x1 / stride-2 conv of a resize unit on the 2x grid
        cin2 = cin * 2 if k == 1 else cin // 2
        x2, w2, b2 = make_conv(rng, n, 2 * ho, 2 * wo, cin2, cout, 1, 8, 8)
        m1, e1 = rand_tables(rng, cout, 2e-4, 3e-3)
        from hawq_amd.packing import pack_ctab
        keep.update(x2=dev(pack_act(x2, 8)), w2=dev(pack_conv_weight(w2, 8)), b2=dev(b2.astype(np.int32)), m1=dev(m1), e1=dev(e1),
                    ctab_id=dev(pack_ctab(b2, m1, e1)))
        a.in2, a.wgt2, a.bias2 = keep['x2'].data_ptr(), keep['w2'].data_ptr(), keep['b2'].data_ptr()
        a.H2, a.W2, a.Cin2, a.stride2, a.in2_bits, a.w2_bits = 2 * ho, 2 * wo, cin2, 2, 8, 8
        a.m_id, a.e_id = keep['m1'].data_ptr(), keep['e1'].data_ptr()
        if TABLES[tables]:
            a.ctab_id = keep['ctab_id'].data_ptr()
    else:
        res = np.full((n, ho, wo, cout), 65500, np.int64) if big_res else rng.integers(0, 60000, (n, ho, wo, cout))
        keep['res'] = dev(res.astype(np.uint16 if res_bits == 16 else np.int32))
        m1, e1 = requant_table(torch.tensor([0.37 * 0.7]), torch.ones(1), torch.tensor([0.7]))
        if big_res:
            m1, e1 = np.array([1 << 30], np.int32), np.array([33 | (3 << 8)], np.int32)   # ratio 1: 65500 + conv > 65535 somewhere
        a.res_in, a.res_in_bits, a.m_id_scalar, a.e_id_scalar = keep['res'].data_ptr(), res_bits, int(m1[0]), int(e1[0])
    mq, eq = requant_table(torch.tensor([0.0039 * 0.7]), torch.ones(1), torch.tensor([0.7]))
    a.out_bits, a.q_lo, a.q_hi, a.mq, a.eq = 8, 0, 127, int(mq[0]), int(eq[0])
    t = _outputs(a, n * ho * wo, cout, res_bits)
    return a, keep, t, x


@pytest.mark.parametrize("layout", ["nhwc", "planar"])
@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("layer,n", [("resnet18.stage4.conv2", 1), ("resnet50.stage4.conv3", 3), ("resnet50.stage3.conv2", 16)])
def test_residual_passthrough_is_byte_identical_to_hawq_conv2d(lib, layer, n, tables, layout):
    if layout == "planar" and not TABLES[tables]:
        return
    a, keep, t, x = _residual_case(lib, np.random.default_rng(21 + n), layer, n, tables, dual=False)
    if layout == "planar":
        a.out_planar = 1
        keep['xp'] = dev(to_planar(pack_act(x, 8)))
    _compare_with_conv2d(lib, a, t, keep.get('xp'), expect_flag=0)


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("layer,n", [("resnet50.stage4.conv3", 1), ("resnet50.stage4.conv3", 16), ("resnet18.stage4.conv2", 3),
                                     ("resnet18.stage4.conv2", 1)])
def test_residual_with_identity_conv_is_byte_identical_to_hawq_conv2d(lib, layer, n, tables):
    # resnet50: unitN.conv3 (1x1, K 512) + identity (1x1 / 2, K 1024); resnet18: conv2 (3x3, K 4608) + identity (1x1 / 2, K 256)
    a, keep, t, _ = _residual_case(lib, np.random.default_rng(31 + n), layer, n, tables, dual=True)
    assert _compare_with_conv2d(lib, a, t)


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("res_bits", [16, 32])
def test_residual_overflow_bit_is_set_as_hawq_conv2d_sets_it(lib, tables, res_bits):
    a, keep, t, _ = _residual_case(lib, np.random.default_rng(41), "resnet18.stage4.conv2", 1, tables, dual=False,
                                   res_bits=res_bits, big_res=True)
    _compare_with_conv2d(lib, a, t, expect_flag=1 if res_bits == 16 else 0)


def test_counters_reset_back_to_back_launches_and_graph_replay(lib):
    a, keep, t, _ = _residual_case(lib, np.random.default_rng(51), "resnet50.stage4.conv3", 1, "fast", dual=True)
    lib.call("hawq_conv2d", C.byref(a), stream())
    ref = _snapshot(t)
    s = 4
    ws = workspace(lib, a, s)
    for _ in range(10):
        splitk(lib, a, s, ws)
    torch.cuda.synchronize()
    assert int(ws[1].abs().sum()) == 0
    got = _snapshot(t)
    assert all(np.array_equal(got[k], ref[k]) for k in ref)
    st = torch.cuda.Stream()
    g = C.c_void_p()
    with torch.cuda.stream(st):
        lib.call("hawq_graph_begin", st.cuda_stream)
        try:
            lib.call("hawq_conv2d_splitk", C.byref(a), s, ws[0].data_ptr(), ws[1].data_ptr(), st.cuda_stream)
        finally:
            lib.call("hawq_graph_end", st.cuda_stream, C.byref(g))
        for v in t.values():
            v.zero_()
        for _ in range(3):
            lib.call("hawq_graph_launch", g, st.cuda_stream)
    st.synchronize()
    lib.call("hawq_graph_destroy", g)
    assert int(ws[1].abs().sum()) == 0
    got = _snapshot(t)
    assert all(np.array_equal(got[k], ref[k]) for k in ref)
