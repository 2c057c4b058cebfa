"""InceptionV3's fused fp32 stem, host side (no GPU): the launch contract of hawq_incep_stem_f32 (hawq_incep_stem_f32_ok launches
nothing and dereferences nothing), its declaration and export, and the engine argument."""
import ctypes
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _good_args():
    """a valid conv1 description (that of tests/test_inception_uint8_host.py); the pointers are never dereferenced by the _ok query"""
    from hawq_amd import _lib
    a = _lib.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = None, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = 2, 299, 299, 3, 32, 3, 3, 2, 0, 0
    a.epilogue, a.relu, a.q_lo, a.q_hi, a.out_bits, a.ldo, a.c_off = _lib.INCEP_REQUANT, 1, -128, 127, 8, 32, 0
    return a


def _ok(a, x=0x60000, inv=37.5, lo=-128, hi=127):
    from hawq_amd import _lib
    return _lib.load().hawq_incep_stem_f32_ok(x, inv, lo, hi, ctypes.byref(a) if a is not None else None)


def test_stem_f32_ok_accepts_conv1():
    assert _ok(_good_args()) == 1
    for ldo, c_off, cout, lo, hi in ((48, 16, 32, 0, 15), (16, 0, 16, -8, 7), (64, 0, 48, 0, 127)):
        a = _good_args()
        a.ldo, a.c_off, a.Cout, a.q_lo, a.q_hi = ldo, c_off, cout, lo, hi
        assert _ok(a) == 1, (ldo, c_off, cout)
    a = _good_args()
    a.H, a.W = 3, 3
    assert _ok(a) == 1
    a = _good_args()
    a.H, a.W = 4, 300   # even sizes: the last input row and column are never read
    assert _ok(a) == 1
    assert _ok(_good_args(), lo=-8, hi=7) == 1 and _ok(_good_args(), lo=0, hi=0) == 1
    assert _ok(_good_args(), inv=1e-30) == 1 and _ok(_good_args(), x=0x60004) == 1   # any positive finite scale, dword alignment


def test_stem_f32_ok_refuses_each_field_changed_alone():
    assert _ok(None) == 0
    assert _ok(_good_args(), x=None) == 0
    assert _ok(_good_args(), x=0x60002) == 0   # the images are read as dwords
    bad = {
        "in_": 0x80000, "wgt": None, "bias": None, "out": None, "m": None, "ek": None,
        "N": 0, "H": 2, "W": 2, "Cin": 16, "Cout": 24, "KH": 5, "KW": 1, "stride": 1, "pad_h": 1, "pad_w": 1,
        "epilogue": 0, "out_bits": 16, "q_lo": -129, "q_hi": 128, "ldo": 24, "c_off": 8,
    }
    for field, value in bad.items():
        a = _good_args()
        setattr(a, field, value)
        assert _ok(a) == 0, field
    a = _good_args()
    a.epilogue = 2   # REQUANT2
    assert _ok(a) == 0
    a = _good_args()
    a.q_lo, a.q_hi = 5, 4
    assert _ok(a) == 0
    a = _good_args()
    a.ldo, a.c_off = 32, 16   # the slice would run past the row
    assert _ok(a) == 0
    a = _good_args()
    a.out = 0x30008   # the 16-byte stores need an aligned output
    assert _ok(a) == 0
    a = _good_args()
    a.wgt = 0x10008   # the weight fragment is one 16-byte load
    assert _ok(a) == 0
    a = _good_args()
    a.N, a.H, a.W = 1 << 16, 1 << 10, 1 << 10   # more than 2^31 output pixels
    assert _ok(a) == 0
    # the input QuantAct's arguments
    for inv in (0.0, -37.5, -0.0, math.inf, -math.inf, math.nan):
        assert _ok(_good_args(), inv=inv) == 0, inv
    assert _ok(_good_args(), lo=-129) == 0
    assert _ok(_good_args(), hi=128) == 0
    assert _ok(_good_args(), lo=-32768, hi=32767) == 0   # a 16-bit input QuantAct
    assert _ok(_good_args(), lo=5, hi=4) == 0


def test_launch_reports_the_refusal_without_a_device():
    """hawq_incep_stem_f32 checks the description before it touches the device: the reason ends up in hawq_last_error()"""
    from hawq_amd import _lib
    L = _lib.load()
    a = _good_args()
    a.Cin = 16
    assert L.hawq_incep_stem_f32(0x60000, 37.5, -128, 127, ctypes.byref(a), None) != 0
    msg = L.hawq_last_error().decode()
    assert "hawq_incep_stem_f32" in msg and "3 channels in" in msg
    assert L.hawq_incep_stem_f32(0x60000, math.nan, -128, 127, ctypes.byref(_good_args()), None) != 0
    assert "inv_scale" in L.hawq_last_error().decode()


def test_header_declares_and_library_exports_both_symbols():
    from hawq_amd import _lib
    header = open(os.path.join(ROOT, "include", "hawq_mi355.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int hawq_incep_stem_f32(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, "
            "const hawq_incep_conv_args *conv, void *stream);") in flat
    assert ("int hawq_incep_stem_f32_ok(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, "
            "const hawq_incep_conv_args *conv);") in flat
    assert "#define HAWQ_ABI_VERSION 5" in header
    L = _lib.load()
    assert L.hawq_abi_version() == 5
    raw = ctypes.CDLL(_lib.library_path())   # the library built here, not the binding's table
    for name in ("hawq_incep_stem_f32", "hawq_incep_stem_f32_ok"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["hawq_incep_stem_f32"]) == len(_lib.SIGNATURES["hawq_incep_stem_f32_ok"]) + 1 == 6


def test_engine_takes_and_stores_the_flag_without_a_device():
    from hawq_amd.api import build_quantized_resnet
    from hawq_amd.engine_inception import InceptionEngine
    q = build_quantized_resnet("inceptionv3", "uniform8", seed=None)
    eng = InceptionEngine(q, fused_stem=True)
    assert eng.fused_stem is True and eng.stream is None and eng.n_launches == 0
    assert InceptionEngine(q).fused_stem is False
    assert InceptionEngine(q, fused_stem=1, tune=True, fast_pools=True, use_graph=False).fused_stem is True
    assert q.engine(fused_stem=True).fused_stem is True          # Q_InceptionV3.engine passes keywords through
    q.invalidate_engine()
    assert q.engine().fused_stem is False
    # the model-level refusal both one-launch stem kernels share
    ib = q.features.q_init_block
    assert InceptionEngine._stem_refusal(ib) is None
    ib.q_input_activ.activation_bit = 16
    assert "input QuantAct" in InceptionEngine._stem_refusal(ib)
