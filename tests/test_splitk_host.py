"""Host-side contract of the split-K conv entry points (hawq_conv2d_splitk_ok / hawq_conv2d_splitk_workspace): which launches the
kernel takes, and the workspace it needs.  Host-only functions, called through ctypes: no GPU needed."""
import ctypes as C

import pytest

from hawq_amd import _lib

CANDIDATES = (2, 4, 8, 16, 32)
# hawq_conv2d_num_tiles() of the library before split-K existed: the split-K kernel adds no tile id, so recorded plans stay valid
NUM_CONV_TILES = 28


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def args(n, h, w, cin, cout, k, stride, epi=_lib.EPI_REQUANT, **kw):
    a = _lib.ConvArgs()
    a.in_, a.wgt, a.bias = 16, 16, 16   # never dereferenced by the host-only queries
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = n, h, w, cin, cout, k, k, stride, k // 2
    a.in_bits, a.w_bits, a.epilogue = 8, 8, epi
    if epi == _lib.EPI_REQUANT:
        a.out_q, a.out_bits, a.relu = 16, 8, 1
    elif epi == _lib.EPI_RESIDUAL:
        a.out_q, a.out_bits, a.res_out, a.res_out_bits, a.res_in, a.res_in_bits = 16, 8, 16, 16, 16, 16
    elif epi == _lib.EPI_RAW:
        a.out_acc = 16
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def ok(lib, a, s):
    return lib.hawq_conv2d_splitk_ok(C.byref(a), s)


def stage4_3x3(**kw):
    return args(1, 7, 7, 512, 512, 3, 1, **kw)   # ResNet50 stage 4 conv2 at batch 1: M = 49, K = 9 * 512 = 72 chunks


def stage3_conv3_identity(n=1):
    # ResNet50 stage-3 unit 1: conv3 (1x1, 256 -> 1024 on 14x14) + identity conv (1x1 / 2, 512 -> 1024 from 28x28)
    return args(n, 14, 14, 256, 1024, 1, 1, epi=_lib.EPI_RESIDUAL, res_in=None, res_in_bits=0, in2=16, wgt2=16, bias2=16,
                H2=28, W2=28, Cin2=512, stride2=2, in2_bits=8, w2_bits=8, m_id=16, e_id=16)


def test_entry_points_are_declared_and_the_abi_is_unchanged(lib):
    for name in ("hawq_conv2d_splitk_ok", "hawq_conv2d_splitk_workspace", "hawq_conv2d_splitk"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.hawq_abi_version() == 5
    assert lib.hawq_conv2d_num_tiles() == NUM_CONV_TILES


def test_takes_the_resnet50_stage4_3x3_at_batch_1(lib):
    a = stage4_3x3()
    taken = [s for s in CANDIDATES if ok(lib, a, s)]
    # every candidate that divides the 72 K chunks (64 input channels of one tap each)
    assert taken == [s for s in CANDIDATES if 72 % s == 0] == [2, 4, 8]
    for epi in (_lib.EPI_RAW, _lib.EPI_REQUANT, _lib.EPI_RESIDUAL):
        assert ok(lib, stage4_3x3(epi=epi), 8)
    assert ok(lib, stage4_3x3(in_planar=1, fast_tables=1), 4) and ok(lib, stage4_3x3(out_planar=1, fast_tables=1), 4)
    assert ok(lib, args(1, 14, 14, 512, 512, 3, 2), 8)      # ResNet50b's strided 3x3
    assert ok(lib, args(1, 14, 14, 1024, 512, 1, 2), 16)    # strided 1x1, K = 16 chunks


def test_takes_a_stage3_conv3_with_its_identity_conv(lib):
    a = stage3_conv3_identity()
    assert [s for s in CANDIDATES if ok(lib, a, s)] == [2, 4]   # 4 K chunks in the main branch


@pytest.mark.parametrize("field,value", [("in_bits", 4), ("w_bits", 4), ("out_bits", 4), ("n_valid", 500), ("in_pitch", 256),
                                         ("out_pitch", 256), ("epilogue", _lib.EPI_DEQUANT)])
def test_refuses_what_it_does_not_implement(lib, field, value):
    a = stage4_3x3()
    assert ok(lib, a, 2)
    setattr(a, field, value)
    assert not ok(lib, a, 2)


def test_refuses_other_forms(lib):
    assert not ok(lib, stage4_3x3(), 16) and not ok(lib, stage4_3x3(), 5) and not ok(lib, stage4_3x3(), 1)
    assert not ok(lib, args(1, 14, 14, 256, 256, 5, 1), 2)                 # 5x5
    assert not ok(lib, stage4_3x3(in_planar=1, fast_tables=0), 2)         # planar input: fast-contract epilogues only
    a = stage3_conv3_identity()
    a.in2_bits = 4
    assert not ok(lib, a, 2)
    a = stage3_conv3_identity()
    a.epilogue = _lib.EPI_REQUANT
    assert not ok(lib, a, 2)
    rc = lib.hawq_conv2d_splitk_workspace(C.byref(stage4_3x3()), 16, None, None)
    assert rc != 0 and b"do not divide" in lib.hawq_last_error()


def workspace(lib, a, s):
    slab, cnt = C.c_int64(-1), C.c_int64(-1)
    assert lib.hawq_conv2d_splitk_workspace(C.byref(a), s, C.byref(slab), C.byref(cnt)) == 0
    return slab.value, cnt.value


@pytest.mark.parametrize("s", [2, 4, 8])
def test_workspace_follows_the_documented_formula(lib, s):
    # slab = tiles * (S + S2) * 64 * 64 * 4 bytes, counters = tiles * 4 bytes, tiles = ceil(M / 64) * Cout / 64
    tiles = 1 * (512 // 64)
    assert workspace(lib, stage4_3x3(), s) == (tiles * s * 64 * 64 * 4, tiles * 4)
    for n in (1, 3, 16):
        a = args(n, 7, 7, 512, 2048, 1, 1)
        tiles = -(-n * 49 // 64) * 32
        assert workspace(lib, a, s) == (tiles * s * 16384, tiles * 4)


def test_workspace_of_the_identity_branch_slices(lib):
    # main branch 4 chunks; identity 8 chunks in slices of q2 = the largest divisor of 8 that is <= 4 / S chunks
    tiles = -(-196 // 64) * 16
    assert workspace(lib, stage3_conv3_identity(), 2) == (tiles * (2 + 4) * 16384, tiles * 4)
    assert workspace(lib, stage3_conv3_identity(), 4) == (tiles * (4 + 8) * 16384, tiles * 4)
    # ResNet18 conv2 + identity: 3x3 on 256 channels (36 chunks), identity 128 channels (2 chunks, one slice of 2)
    a = args(1, 14, 14, 256, 256, 3, 1, epi=_lib.EPI_RESIDUAL, res_in=None, res_in_bits=0, in2=16, wgt2=16, bias2=16,
             H2=28, W2=28, Cin2=128, stride2=2, in2_bits=8, w2_bits=8, m_id=16, e_id=16)
    tiles = 4 * 4
    assert workspace(lib, a, 4) == (tiles * (4 + 1) * 16384, tiles * 4)
